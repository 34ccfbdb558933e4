"""CPU oracle for VNNGP over the Matern family (TEST INFRASTRUCTURE ONLY, like oracle/svgp_oracle.py).

``oracle.svgp_oracle.vnngp_moments`` (reference gp.py:21-122) with the covariance taken from tests/matern_oracle.py:
nu = 1/2, 3/2 and 5/2, r through the masked square root there, so a datum that coincides with an inducing point (and the
diagonal of Kzz) contributes a zero gradient with respect to the points -- the library's convention -- where the
reference's autograd returns NaN.  Values are unaffected.  Pinned against the reference's own VNNGP run with these
kernels: tests/golden/make_vnngp_matern_golden.py -> extra_vnngp_matern{12,32,52}_{f64,f32}.npz,
tests/test_vnngp_matern.py.

The neighbour table is ranked by ``torch.cdist(X, Z)`` as in the reference (gp.py:31,64: the kernel's
``return_distance``), not by the masked distance.
"""
from __future__ import annotations

import torch
from torch import distributions

import matern_oracle as MO
from oracle import svgp_oracle as O

KINDS = ("matern12", "matern32", "matern52")


def vnngp_moments(kind: str, X, Z, sigma, lengthscale, mu, Lu_raw, jitter: float, K: int, idx=None, with_cov=False):
    """mean, scale (L,N) or (N,), the neighbour indices (N,K), Lu, chol: svgp_oracle.vnngp_moments line by line with
    k = the Matern covariance ``kind``.  ``idx``: a neighbour table to use instead of the argsort.  ``with_cov``: the
    variances before the clamp, (L,N), as a sixth value."""
    batched = sigma.dim() > 0 or lengthscale.dim() > 0
    M = Z.shape[0]
    s = sigma.reshape(-1, 1, 1)
    Kxz = MO.kernel_matrix(kind, X, Z, sigma, lengthscale).reshape(-1, X.shape[0], M)      # (L,N,M)
    Kzz = MO.kernel_matrix(kind, Z, Z, sigma, lengthscale).reshape(-1, M, M)
    Lq = O.lower_cholesky_param(Lu_raw).reshape(-1, M, M)
    chol = torch.linalg.cholesky(O.add_jitter_(Kzz.contiguous(), jitter))
    if idx is None:
        idx = torch.argsort(torch.cdist(X, Z), dim=1)[:, :K]                                # (N,K)
    lL = chol[:, idx]                                                                       # (L,N,K,M)
    lK = lL @ lL.transpose(-2, -1)
    lK = O.add_jitter_(lK.reshape(-1, K, K).contiguous(), jitter).reshape(lK.shape)
    W = (torch.gather(Kxz, 2, idx.expand(Kxz.shape[0], -1, -1))[:, :, None, :] @ torch.inverse(lK))  # (L,N,1,K)
    lmu = mu.reshape(-1, M)[:, idx]                                                         # (L,N,K)
    lLu = Lq[:, idx]
    lS = lLu @ lLu.transpose(-2, -1)
    mean = (W @ lmu[..., None]).squeeze(-1).squeeze(-1)
    cov = s.reshape(-1, 1) ** 2 + ((W @ (lS - lK)) * W).sum(-1).squeeze(-1)
    scale = cov.clamp(min=5e-2) ** 0.5
    if not batched:
        mean, scale = mean[0], scale[0]
    out = (mean, scale, idx, O.lower_cholesky_param(Lu_raw), chol if batched else chol[0])
    return out + (cov,) if with_cov else out


def neg_elbo(kind, X, y, Z, sigma, lengthscale, mu, Lu_raw, jitter, K, noise_sd, idx=None):
    """The loss of test_backward_matches_reference_autograd: -(sum log N(y; mean, s) - sum scale^2 / (2 s^2) - sum KL)."""
    mean, scale, _, Lu, chol = vnngp_moments(kind, X, Z, sigma, lengthscale, mu, Lu_raw, jitter, K, idx=idx)
    kl = distributions.kl_divergence(distributions.MultivariateNormal(mu, scale_tril=Lu),
                                     distributions.MultivariateNormal(torch.zeros_like(mu), scale_tril=chol))
    s = float(noise_sd)
    return -(distributions.Normal(mean, s).log_prob(y).sum() - (scale ** 2).sum() / (2 * s ** 2) - kl.sum())


def grads(kind, X, y, Z, sigma, lengthscale, mu, Lu_raw, jitter, K, noise_sd, idx=None) -> dict:
    """loss and its gradients with respect to Z, sigma, lengthscale, mu and the raw Lu by torch autograd."""
    leaves = {n: t.detach().clone().requires_grad_(True)
              for n, t in (("Z", Z), ("sigma", sigma), ("lengthscale", lengthscale), ("mu", mu), ("Lu", Lu_raw))}
    loss = neg_elbo(kind, X, y, leaves["Z"], leaves["sigma"], leaves["lengthscale"], leaves["mu"], leaves["Lu"], jitter, K,
                    noise_sd, idx=idx)
    loss.backward()
    out = {"grad_" + n: t.grad for n, t in leaves.items()}
    out["loss"] = loss.detach()
    return out
