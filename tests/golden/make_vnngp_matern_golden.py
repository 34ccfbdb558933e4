#!/usr/bin/env python3
"""Golden vectors for VNNGP with Matern-1/2, -3/2 and -5/2 kernels, produced by the REFERENCE itself (build container only).

    MPLBACKEND=Agg python tests/golden/make_vnngp_matern_golden.py

The reference's VNNGP (gp.py:7-122) asks one thing of its kernel beyond the covariance: ``forward(X, Z,
return_distance=True)`` also returns the distance matrix it ranks the neighbours by (gp.py:31,64).  Its Matern-3/2 has
no such argument, so this script adds it -- ``torch.cdist(X, Z)``, exactly what the reference's RBF returns
(kernels.py:118,125-126), the one line a user would add -- to ``batched_Matern32`` and to the nu = 1/2 and nu = 5/2
subclasses of make_matern_golden.py, runs the reference's VNNGP on the recipe of the existing VNNGP fixtures
(make_golden.py's vnngp_cases: seeded inputs, d=2, L=3, M=36, jitter 1e-2, noise 0.5; here N=240, K=10, sigma =
(1.0, 0.8, 1.3), lengthscale = (2.5, 4.0, 6.0), fp64 and fp32) with the loss of
tests/test_hip_vnngp.py::test_backward_matches_reference_autograd and stores inputs + outputs -- data only -- as

    extra_vnngp_matern{12,32,52}_{f64,f32}.npz     X, y, Z, mu, Lu_raw, sigma, lengthscale, jitter, K, noise_sd, idx, mean, scale,
                                                    Lu, chol, loss and the reference autograd gradients of the loss w.r.t.
                                                    mu, Lu, sigma, lengthscale

The reference's grad_Z is NaN (sqrt at r = 0 on the diagonal of k(Z, Z)): asserted, not stored.  Gradients with respect
to Z are checked against tests/vnngp_matern_oracle.py, which takes r through a masked square root.

What the tests rely on is asserted here, and no fixture is written that fails one of these: every stored array finite;
distinct points of X u Z at least 1e-3 min(lengthscale) apart; the reference's neighbour table equal to the (fp64
squared distance, index) ranking, with the gap between a row's K-th and (K+1)-th distance above the reference's own
distance error in that row (so gpz_knn must reproduce ``idx`` exactly); no variance within 1e-6 relative of the 5e-2
clamp.  A seed that fails is skipped for the next one (the seed used is stored).
"""
import contextlib
import io
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, "/root/reference")

import numpy as np
import torch
import torch.nn as nn
from torch import distributions

import gpzoo.gp as rgp          # noqa: E402  (the reference)
import gpzoo.kernels as rk      # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                     # tests/: the oracles
sys.path.insert(1, os.path.dirname(os.path.dirname(HERE)))   # the repository root: oracle/ (gpzoo is already the reference's)
from inputs import make_inputs  # noqa: E402
from make_matern_golden import Matern12, Matern52, assert_separated, vec  # noqa: E402  (nothing runs on import)
import vnngp_matern_oracle as VO  # noqa: E402


class _WithDistance:
    """forward(..., return_distance=True) -> (K, torch.cdist(X, Z)): what the reference's RBF family returns."""

    def forward(self, X, Z, diag=False, return_distance=False):
        K = super().forward(X, Z, diag=diag)
        return (K, torch.cdist(X, Z)) if return_distance else K


class VMatern12(_WithDistance, Matern12):
    pass


class VMatern32(_WithDistance, rk.batched_Matern32):
    pass


class VMatern52(_WithDistance, Matern52):
    pass


CLASSES = {"matern12": VMatern12, "matern32": VMatern32, "matern52": VMatern52}
SIGMA, ELL = [1.0, 0.8, 1.3], [2.5, 4.0, 6.0]
N, M, L, K, JITTER, NOISE = 240, 36, 3, 10, 1e-2, 0.5


def check_table(X, Z, idx, dist_ref):
    """idx == the stable (fp64 squared distance, index) ranking of the (rounded) inputs, and the K / K+1 gap of every row
    exceeds twice the largest error of the reference's own distances in that row."""
    d2 = ((X.double()[:, None, :] - Z.double()[None, :, :]) ** 2).sum(-1)
    order = torch.argsort(d2, dim=1, stable=True)
    assert torch.equal(order[:, :K], idx), "neighbour table differs from the fp64 ranking"
    true = d2.sqrt()
    err = (dist_ref.double() - true).abs().max(dim=1).values
    srt = torch.gather(true, 1, order)
    gap = srt[:, K] - srt[:, K - 1]
    assert bool((gap > 2 * err).all()), f"K / K+1 gap {float((gap - 2 * err).min()):.3e} below the distance error"
    inner = (srt[:, 1:K + 1] - srt[:, :K]).min(dim=1).values
    assert bool((inner > 2 * err).all()), "two of a row's first K + 1 distances lie within the distance error"


def run(kind, dtype, seed):
    inp = make_inputs(seed, N=N, M=M, d=2, L=L)
    X = inp["X"].to(dtype)
    assert_separated(min(ELL), X=X, Z=inp["Z"].to(dtype))
    kern = CLASSES[kind]()
    kern.sigma, kern.lengthscale = vec(SIGMA), vec(ELL)
    gp = rgp.VNNGP(kern, dim=2, M=M, K=K, jitter=JITTER)
    gp.Z = nn.Parameter(inp["Z"].clone()); gp.mu = nn.Parameter(inp["mu"].clone()); gp.Lu = nn.Parameter(inp["Lu_raw"].clone())
    gp = gp.double() if dtype == torch.float64 else gp.float()
    y = inp["y"].to(dtype)
    with contextlib.redirect_stdout(io.StringIO()):          # the reference prints shapes unconditionally
        with torch.no_grad():
            qF, qU, pU = gp(X)
            _, dist = kern(X, gp.Z, return_distance=True)
        idx = torch.argsort(dist, dim=1)[:, :K]
        qF_g, qU_g, pU_g = gp(X)
    loss = -(distributions.Normal(qF_g.mean, NOISE).log_prob(y).sum() - (qF_g.scale ** 2).sum() / (2 * NOISE ** 2)
             - distributions.kl_divergence(qU_g, pU_g).sum())
    loss.backward()
    assert torch.isnan(gp.Z.grad).any(), "the reference's grad_Z was expected to be NaN"
    check_table(X, gp.Z.detach(), idx, dist)
    # the variances before the clamp, by the oracle in fp64 on the same (rounded) inputs
    dd = lambda t: t.detach().double()      # noqa: E731
    cov = VO.vnngp_moments(kind, dd(X), dd(gp.Z), dd(kern.sigma), dd(kern.lengthscale), dd(gp.mu), dd(gp.Lu), JITTER, K,
                           idx=idx, with_cov=True)[5]
    assert float(((cov - 5e-2).abs() / 5e-2).min()) > 1e-6, "a variance sits on the clamp"
    rec = dict(X=X.numpy(), y=y.numpy(), Z=gp.Z.detach().numpy(), mu=gp.mu.detach().numpy(), Lu_raw=gp.Lu.detach().numpy(),
               sigma=kern.sigma.detach().numpy(), lengthscale=kern.lengthscale.detach().numpy(),
               idx=idx.numpy(), mean=qF.mean.numpy(), scale=qF.scale.numpy(), Lu=qU.scale_tril.numpy(),
               chol=pU.scale_tril.numpy(), loss=np.float64(float(loss.detach())), grad_mu=gp.mu.grad.numpy(),
               grad_Lu=gp.Lu.grad.numpy(), grad_sigma=kern.sigma.grad.numpy(), grad_lengthscale=kern.lengthscale.grad.numpy())
    for k, v in rec.items():
        assert np.isfinite(v).all(), k
    rec.update(jitter=np.float64(JITTER), K=np.int64(K), noise_sd=np.float64(NOISE), seed=np.int64(seed),
               n_clamped=np.int64(int((cov <= 5e-2).sum())), kind=np.array(kind))
    return rec


def main():
    for i, kind in enumerate(CLASSES):
        for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            last = None
            for seed in range(900 + 20 * i, 900 + 20 * i + 20):
                try:
                    rec = run(kind, dtype, seed)
                    break
                except AssertionError as e:
                    last = e
            else:
                raise SystemExit(f"{kind} {tag}: no seed passed ({last})")
            path = os.path.join(HERE, f"extra_vnngp_{kind}_{tag}.npz")
            np.savez_compressed(path, **rec)
            assert os.path.getsize(path) < 512 * 1024, path
            print(f"extra_vnngp_{kind}_{tag}: seed={seed} loss={float(rec['loss']):.8f} clamped={int(rec['n_clamped'])} "
                  f"bytes={os.path.getsize(path)}")


if __name__ == "__main__":
    torch.manual_seed(0)
    main()
