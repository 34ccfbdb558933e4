#!/usr/bin/env python
"""Generate the project_factors_to_inducing golden vectors by running the notebooks' composition on the REFERENCE's own
kernels (build container, CPU only, fp64).

    python tests/golden/make_projection_golden.py

writes tests/golden/extra_projection_<case>.npz -- the ``extra_`` prefix keeps them out of conftest.golden_cases().  Data
only.

The composition is Slideseqv2_estimate_lengthscales.ipynb's ``build_model_scracth``:

    Kzx = kernel(Z, X); Kzz = kernel(Z, Z)
    L1 = cholesky(add_jitter(Kzx @ Kxz, 1e-5)); alpha = cholesky_solve(Kzx @ F, L1); mu = Kzz @ alpha

with the reference's ``RBF``, ``NSF_RBF``, ``batched_RBF`` and ``batched_Matern32`` and its ``add_jitter``.  Inputs come
from tests/projection_cases.recipe (float32-representable numbers, run here as float64).  Per case: the inputs, ``mu``,
``alpha`` (L, M), ``b`` (L, M), ``cond`` = the 2-norm condition number of G + jitter I (the largest over the latents) and
``ref32_err`` = the relative max-norm error of mu when the same composition runs in float32, against its own float64 run.
G itself is not stored (1 MB at M = 257).  A case is written only if cond <= 1e4 and ref32_err <= 1e-4."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, "/root/reference")
import gpzoo.kernels as rk                       # noqa: E402  (the reference)
from gpzoo.utilities import add_jitter           # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import projection_cases as PC  # noqa: E402

JITTER = 1e-5


def make_kernel(cls, sigma, ell, L, dtype):
    s, e = torch.as_tensor(sigma, dtype=dtype), torch.as_tensor(ell, dtype=dtype)
    if cls == "NSF_RBF":
        k = rk.NSF_RBF(L=L)
        k.sigma.data, k.lengthscale.data = s.reshape(L, 1, 1).clone(), e.reshape(L, 1, 1).clone()
        return k
    k = getattr(rk, cls)()
    k.sigma.data, k.lengthscale.data = s.clone(), e.clone()
    return k


def compose(kernel, Z, X, F, per_latent):
    """The notebook's lines; returns mu, alpha, b as (L, M) and G + jitter I as (n, M, M)."""
    with torch.no_grad():
        Kzx, Kzz = kernel(Z, X), kernel(Z, Z)
        G = add_jitter(Kzx @ torch.transpose(Kzx, -1, -2), JITTER)
        L1 = torch.linalg.cholesky(G)
        b = Kzx @ (F[:, :, None] if per_latent else F.t())           # (L, M, 1) / (M, L)
        alpha = torch.cholesky_solve(b, L1)
        mu = Kzz @ alpha
    flat = (lambda t: t[:, :, 0]) if per_latent else (lambda t: t.t())
    return flat(mu), flat(alpha), flat(b), (G if per_latent else G[None])


def make(name):
    N, M, L, frac, cls, per_latent = PC.GOLDENS[name]
    for seed in range(100):
        inp = PC.recipe(N, M, L, frac, seed, per_latent=per_latent)
        run = {}
        for dt in (torch.float64, torch.float32):
            kernel = make_kernel(cls, inp["sigma"], inp["lengthscale"], L, dt)
            Z, X, F = (torch.as_tensor(inp[k]).to(dt) for k in ("Z", "X", "F"))
            try:
                run[dt] = compose(kernel, Z, X, F, per_latent)
            except torch.linalg.LinAlgError:
                run[dt] = None
        if run[torch.float32] is None:
            continue
        mu, alpha, b, G = run[torch.float64]
        cond = float(torch.linalg.cond(G).max())
        err32 = float((run[torch.float32][0].double() - mu).abs().max() / mu.abs().max())
        if not (cond <= PC.COND_MAX and err32 <= PC.REF32_ERR_MAX):
            continue
        np.savez_compressed(os.path.join(HERE, f"extra_projection_{name}.npz"), X=inp["X"], Z=inp["Z"], F=inp["F"],
                            sigma=inp["sigma"], lengthscale=inp["lengthscale"], jitter=JITTER, mu=mu.numpy(), alpha=alpha.numpy(),
                            b=b.numpy(), cond=cond, ref32_err=err32, data_seed=seed, frac=frac)
        print(f"{name}: data seed {seed}, cond {cond:.3g}, ref32_err {err32:.3g}", flush=True)
        return
    raise SystemExit(f"{name}: no draw held the conditions")


if __name__ == "__main__":
    for name in PC.GOLDENS:
        make(name)
