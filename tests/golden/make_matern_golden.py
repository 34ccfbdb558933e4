#!/usr/bin/env python3
"""Golden vectors for the Matern-1/2 and Matern-5/2 kernels, produced by the REFERENCE itself (build container only).

    MPLBACKEND=Agg python tests/golden/make_matern_golden.py

The reference ships Matern-3/2 only, but its vmap kernels evaluate an overridable ``covariance(x1, x2)``
(kernels.py:14-20, 29): a user who wants another smoothness subclasses ``batched_Matern32`` and writes the closed form.
This script does exactly that for nu = 1/2 and nu = 5/2, runs the reference's WSVGP / SVGP + ExactLikelihood with those
subclasses on make_golden.py's Matern-3/2 recipe (N=160, M=36, d=2, L=3, sigma = (1.0, 0.8, 1.3), lengthscale =
(2.5, 4.0, 6.0), jitter 1e-2, noise 0.5, fp64 and fp32) and stores inputs + outputs -- data only -- as

    extra_matern{12,52}_{wsvgp,svgp}_{f32,f64}.npz     inputs, Kzx, Kzz_jit, chol, mean, scale, Lu, kl, elbo and the
                                                        reference autograd gradients of -ELBO w.r.t. mu, Lu, sigma, lengthscale
    extra_matern_kernels_only.npz                       k(Z, X) at 77 x 96 with scalar and vector parameters, and k(Z, Z)

The reference's grad_Z is NaN (sqrt at r = 0 on the diagonal of k(Z, Z)), so it is not stored: gradients with respect
to points are checked against tests/matern_oracle.py, which takes r through a masked square root.

Every fixture is asserted to keep distinct points at least 1e-3 min(lengthscale) apart: below that the fp32 unit vector
(z - x) / r of the nu = 1/2 gradient is ill-conditioned, and the fixtures must not depend on it.
"""
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, "/root/reference")

import numpy as np
import torch
import torch.nn as nn

import gpzoo.gp as rgp          # noqa: E402  (the reference)
import gpzoo.kernels as rk      # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from inputs import make_inputs  # noqa: E402
from make_golden import run_case  # noqa: E402  (the shared evaluation of a reference model; nothing runs on import)


class Matern12(rk.batched_Matern32):
    def covariance(self, x1, x2):
        dist = torch.sqrt(((x1 - x2) ** 2).sum())
        return (self.sigma ** 2) * torch.exp(-dist / self.lengthscale)


class Matern52(rk.batched_Matern32):
    def covariance(self, x1, x2):
        dist = torch.sqrt(((x1 - x2) ** 2).sum())
        val = (5 ** 0.5) * dist / self.lengthscale
        return (self.sigma ** 2) * (1 + val + val * val / 3) * torch.exp(-val)


CLASSES = {"matern12": Matern12, "matern52": Matern52}
SIGMA, ELL = [1.0, 0.8, 1.3], [2.5, 4.0, 6.0]


def assert_separated(ell_min, **sets):
    """No pair of distinct points closer than 1e-3 min(lengthscale), within and across the given point sets."""
    names = list(sets)
    for i, a in enumerate(names):
        for b in names[i:]:
            d = torch.cdist(sets[a].double(), sets[b].double())
            if a == b:
                d = d + torch.diag(torch.full((d.shape[0],), float("inf"), dtype=d.dtype))
            assert float(d.min()) >= 1e-3 * ell_min, f"{a}-{b}: closest pair {float(d.min()):.3e} < {1e-3 * ell_min:.3e}"


def vec(v, dtype=torch.float64):
    return nn.Parameter(torch.tensor(v, dtype=dtype))


def model_cases():
    i = 0
    for kind, cls in CLASSES.items():
        for name, gpc, whitened in (("wsvgp", "WSVGP", True), ("svgp", "SVGP", False)):
            for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
                inp = make_inputs(500 + 10 * i, N=160, M=36, d=2, L=3)
                assert_separated(min(ELL), X=inp["X"].to(dtype), Z=inp["Z"].to(dtype))
                kern = cls()
                kern.sigma, kern.lengthscale = vec(SIGMA), vec(ELL)
                out = run_case(f"{kind}_{name}", getattr(rgp, gpc), kern, inp, dtype, 1e-2, 0.5, whitened, False)
                assert np.isnan(out.pop("grad_Z")).any(), "the reference's grad_Z was expected to be NaN"
                for k in ("grad_mu", "grad_Lu", "grad_sigma", "grad_lengthscale", "Kzx", "chol", "mean", "scale"):
                    assert np.isfinite(out[k]).all(), k
                out["kind"] = np.array(kind); out["whitened"] = np.array(whitened)
                np.savez_compressed(os.path.join(HERE, f"extra_{kind}_{name}_{tag}.npz"), **out)
                print(f"extra_{kind}_{name}_{tag}: elbo={float(out['elbo']):.10f} cond(Kzz)<="
                      f"{max(float(np.linalg.cond(k)) for k in out['Kzz_jit'].astype(np.float64)):.3g}")
            i += 1


def kernel_only_cases():
    out = {}
    inp = make_inputs(582, N=96, M=77, d=2, L=3)     # (a seed at which the separation below holds)
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        X, Z = inp["X"].to(dtype), inp["Z"].to(dtype)
        assert_separated(2.0, X=X, Z=Z)
        out[f"{tag}_X"], out[f"{tag}_Z"] = X.numpy(), Z.numpy()
        for kind, cls in CLASSES.items():
            kv = cls()
            kv.sigma, kv.lengthscale = vec(SIGMA, dtype), vec(ELL, dtype)
            ks = cls(sigma=0.9, lengthscale=2.0).to(dtype)
            with torch.no_grad():
                out[f"{tag}_{kind}_vec"] = kv(Z, X).numpy()          # (3, 77, 96)
                out[f"{tag}_{kind}_scalar"] = ks(Z, X).numpy()       # (77, 96)
                out[f"{tag}_{kind}_zz"] = ks(Z, Z).numpy()           # r = 0 on the diagonal
    np.savez_compressed(os.path.join(HERE, "extra_matern_kernels_only.npz"), **out)
    print(f"extra_matern_kernels_only.npz: {len(out)} arrays")


if __name__ == "__main__":
    torch.manual_seed(0)
    model_cases()
    kernel_only_cases()
