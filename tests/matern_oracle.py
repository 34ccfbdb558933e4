"""CPU oracle for the Matern-1/2 and Matern-5/2 covariances (TEST INFRASTRUCTURE ONLY, like oracle/svgp_oracle.py).

Plain torch CPU ops; the gradient tests differentiate through it with torch autograd.  It restates what a subclass of
the reference's ``batched_Matern32`` evaluates when its ``covariance(x1, x2)`` (kernels.py:14-20) is replaced by one of

    nu = 1/2:  sigma^2 exp(-r / l)
    nu = 5/2:  sigma^2 (1 + v + v^2 / 3) exp(-v),  v = sqrt(5) r / l,          r = ||x1 - x2||

and is pinned against outputs of exactly such subclasses run through the reference (tests/golden/make_matern_golden.py
-> tests/golden/extra_matern*.npz; tests/test_matern_family.py checks every stored array).  Everything that is not the
covariance itself (Cholesky, moments, KL, ELBO) is oracle/svgp_oracle.py's.

One deliberate difference: r is taken through a MASKED square root, so a coincident pair contributes a zero gradient
with respect to the points where the reference's autograd returns NaN (sqrt at 0, as for Matern-3/2).  Zero is the true
derivative for nu = 5/2 and the library's stated value at the kink of nu = 1/2.  Values are unaffected.
"""
from __future__ import annotations

import math

import torch

from oracle import svgp_oracle as O

KINDS = ("matern12", "matern52")


def masked_distance(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """r = ||a - b|| by direct differencing (kernels.py:14-16); d r / d(a, b) = 0 where r = 0."""
    d2 = O.sqdist_direct(A, B)
    pos = d2 > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, d2, torch.ones_like(d2))), torch.zeros_like(d2))


def kernel_matrix(kind: str, A, B, sigma, lengthscale) -> torch.Tensor:
    """K(A, B): (a, b) for scalar parameters, (L, a, b) for length-L ones."""
    s, ell = O._per_latent(sigma), O._per_latent(lengthscale)
    r = masked_distance(A, B)
    if kind == "matern12":
        return s ** 2 * torch.exp(-r / ell)
    if kind == "matern52":
        v = math.sqrt(5.0) * r / ell
        return s ** 2 * (1.0 + v + v * v / 3.0) * torch.exp(-v)
    if kind == "matern32":       # the same masked form of the shipped kernel (a yardstick for the tools)
        v = math.sqrt(3.0) * r / ell
        return s ** 2 * (1.0 + v) * torch.exp(-v)
    raise ValueError(kind)


def covariance(kind: str, x1, x2, sigma, lengthscale) -> torch.Tensor:
    """One pair, as the reference's vmap body sees it."""
    return kernel_matrix(kind, x1.reshape(1, -1), x2.reshape(1, -1), sigma, lengthscale).reshape(
        torch.broadcast_shapes(sigma.shape, lengthscale.shape))


def parts(kind, whitened, X, Z, sigma, lengthscale, mu, Lu_raw, jitter):
    """Kzx, Kzz + jitter I, chol, mean, scale, kl (per latent) in the reference's op order (gp.py:213-228, 270-296)."""
    Kxx = O.kernel_diag(sigma, X.shape[0])
    Kzx = kernel_matrix(kind, Z, X, sigma, lengthscale)
    Kzz = O.add_jitter_(kernel_matrix(kind, Z, Z, sigma, lengthscale).contiguous(), jitter)
    if whitened:
        mean, scale, Lu, chol = O.wsvgp_moments(Kxx, Kzx, Kzz, mu, Lu_raw)
        kl = O.whitened_kl(mu, Lu)
    else:
        mean, scale, Lu, chol = O.svgp_moments(Kxx, Kzx, Kzz, mu, Lu_raw)
        kl = O.mvn_kl(mu, Lu, chol)
    return dict(Kzx=Kzx, Kzz_jit=Kzz, chol=chol, mean=mean, scale=scale, kl=kl, Lu=Lu)


def elbo_eval(kind, whitened, X, y, Z, sigma, lengthscale, mu, Lu_raw, jitter, noise_sd):
    """(elbo fp64 scalar, mean, scale), like svgp_oracle.elbo_eval."""
    p = parts(kind, whitened, X, Z, sigma, lengthscale, mu, Lu_raw, jitter)
    return O.gaussian_elbo(y, p["mean"], p["scale"], noise_sd, p["kl"]), p["mean"], p["scale"]


def neg_elbo(kind, whitened, X, y, Z, sigma, lengthscale, mu, Lu_raw, jitter, noise_sd) -> torch.Tensor:
    """-ELBO in the inputs' own precision (what loss.backward() differentiates, utilities.py:479-485)."""
    p = parts(kind, whitened, X, Z, sigma, lengthscale, mu, Lu_raw, jitter)
    s2 = float(noise_sd) ** 2
    loglik = (-0.5 * math.log(2.0 * math.pi * s2) - (y - p["mean"]) ** 2 / (2.0 * s2)).sum()
    return -(loglik - (p["scale"] ** 2).sum() / (2.0 * s2) - p["kl"].sum())


def grads(kind, whitened, X, y, Z, sigma, lengthscale, mu, Lu_raw, jitter, noise_sd) -> dict:
    """Gradients of -ELBO with respect to Z, sigma, lengthscale, mu and Lu_raw by torch autograd."""
    leaves = {n: t.detach().clone().requires_grad_(True)
              for n, t in (("Z", Z), ("sigma", sigma), ("lengthscale", lengthscale), ("mu", mu), ("Lu", Lu_raw))}
    loss = neg_elbo(kind, whitened, X, y, leaves["Z"], leaves["sigma"], leaves["lengthscale"], leaves["mu"], leaves["Lu"],
                    jitter, noise_sd)
    loss.backward()
    out = {"grad_" + n: t.grad for n, t in leaves.items()}
    out["loss"] = loss.detach()
    return out
