#!/usr/bin/env python3
"""Real-valued spatial factorisation (RSF, the nsf paper's Gaussian model, i.e. MEFISTO) on synthetic normalised
expression: smooth signed factors on a 2-D tissue, real loadings, an intercept and one noise level per gene; ``RSF`` over a
whitened SVGP prior, fitted with ``train_batched`` through the fused exact step (``gpz_gaussian_fa``: no samples), then
``model.score`` on held-out spots.

With ``--sparse-expression DENSITY`` the data are counts instead, held as their non-zeros from start to end: synthetic
Poisson counts with about DENSITY of the entries non-zero -> ``SparseCounts`` -> ``train_val_split`` -> ``log_normalize``
(log1p of size-normalised counts, centred per gene; the held-out split is centred with the training split's offset) ->
the same fit through ``gpz_gaussian_fa_sparse`` -> held-out ``score``.  No (genes, spots) array exists on the device.

With ``--residual-autocorr`` the fit is followed by ``model_residual_autocorr`` on the fitted spots: is spatial structure left
in what the fit did not explain, and in which genes -- the ten genes with the largest z (the smallest for Geary's C), or with
``--residual-perms P`` those with the smallest permutation p-value, each with its ``fdr_bh`` value.  With
``--sparse-expression`` it runs from the ``SparseExpression``.

    PYTHONPATH=. python examples/rsf_synthetic.py [--spots 20000 --genes 1000 --factors 6 --inducing 500 --steps 300]
                                                  [--sparse-expression 0.05]
                                                  [--residual-autocorr [--residual-perms 99] [--residual-mode geary]]
"""
import argparse
import math
import time

import torch
import torch.nn as nn

from gpzoo.gp import WSVGP
from gpzoo.kernels import NSF_RBF
from gpzoo.likelihoods import RSF, SparseCounts, model_residual_autocorr
from gpzoo.utilities import fdr_bh, log_normalize, train_batched, train_val_split


def synthetic_expression(N, D, L, gen):
    """Smooth signed factors (differences of Gaussian bumps), real loadings, per-gene intercept and noise level."""
    X = (torch.rand(N, 2, generator=gen) - 0.5) * 200.0
    c = (torch.rand(2, L, 2, generator=gen) - 0.5) * 160.0
    bump = lambda ctr: torch.exp(-((X[None] - ctr[:, None]) ** 2).sum(-1) / (2 * 35.0 ** 2))  # noqa: E731
    F = bump(c[0]) - bump(c[1])                                                              # (L,N)
    W = torch.randn(D, L, generator=gen)
    b = 2.0 + torch.randn(D, generator=gen)
    sd = 0.2 + 0.8 * torch.rand(D, generator=gen)
    Y = b[:, None] + W @ F + sd[:, None] * torch.randn(D, N, generator=gen)
    return X, Y, sd


def synthetic_counts(N, D, L, density, gen):
    """Poisson counts over smooth non-negative factors, their mean rate set so that about ``density`` of the entries are
    non-zero; the spots come in random order, as ``train_val_split`` assumes."""
    X = (torch.rand(N, 2, generator=gen) - 0.5) * 200.0
    c = (torch.rand(L, 2, generator=gen) - 0.5) * 160.0
    F = torch.exp(-((X[None] - c[:, None]) ** 2).sum(-1) / (2 * 35.0 ** 2))                   # (L,N)
    rate = torch.rand(D, L, generator=gen) ** 2 @ F + 0.02
    rate *= -math.log1p(-density) / float(rate.mean())
    return X, torch.poisson(rate, generator=gen)


def sparse_expression_data(a, gen, dev):
    """(X, expr) of the training split and of the held-out split, both on the device."""
    X, counts = synthetic_counts(a.spots, a.genes, a.factors, a.sparse_expression, gen)
    counts = SparseCounts(counts)
    print(f"{counts.nnz} non-zeros, density {counts.nnz / (a.spots * a.genes):.3f}")
    tr, val = train_val_split(X, counts, train_frac=1.0 - a.holdout, sz="scanpy")
    fit = log_normalize(tr["y"], size_factors=tr["sz"])
    held = log_normalize(val["y"], size_factors=val["sz"], offset=fit.offset)      # centred with the training means
    return tr["X"].to(dev), fit.to(dev), val["X"].to(dev), held.to(dev)


def report_residual_autocorr(model, X, Y, a):
    """The ten genes whose residuals are the most autocorrelated over the fitted spots' 6-nearest-neighbour graph."""
    geary = a.residual_mode == "geary"
    r = model_residual_autocorr(model, X, Y, mode=a.residual_mode, assumption="randomisation", n_perms=a.residual_perms)
    stat = r.C if geary else r.I
    if a.residual_perms is None:
        p = torch.distributions.Normal(0.0, 1.0).cdf(r.z if geary else -r.z)     # one-sided, positive autocorrelation
        order, label = torch.argsort(r.z, descending=not geary), "p (normal approximation of z)"
    else:
        p = r.pval_less if geary else r.pval_greater
        order, label = torch.argsort(p, stable=True), f"p ({a.residual_perms} permutations)"
    q = fdr_bh(p)
    print(f"residual {'Geary C' if geary else 'Moran I'}: median {float(stat.median()):.4f}, expected {float(r.expected):.4f}; "
          f"residual variance, median {float(r.residual_var.median()):.3f}")
    print(f"  gene   {'C' if geary else 'I'}        z       {label}   fdr_bh")
    for g in order[:10].tolist():
        print(f"  {g:5d}  {float(stat[g]):7.4f}  {float(r.z[g]):7.2f}  {float(p[g]):.3g}  {float(q[g]):.3g}")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--spots", type=int, default=20000)
    ap.add_argument("--genes", type=int, default=1000)
    ap.add_argument("--factors", type=int, default=6)
    ap.add_argument("--inducing", type=int, default=500)
    ap.add_argument("--batch", type=int, default=7000)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--holdout", type=float, default=0.1, help="fraction of the spots held out for the score")
    ap.add_argument("--lr", type=float, default=2e-2, help="Adam's learning rate")
    ap.add_argument("--sparse-expression", type=float, default=None, metavar="DENSITY",
                    help="fit log-normalised synthetic counts of this density, held as their non-zeros (SparseExpression)")
    ap.add_argument("--residual-autocorr", action="store_true",
                    help="after the fit, score the spatial autocorrelation of every gene's residuals over the fitted spots")
    ap.add_argument("--residual-perms", type=int, default=None, metavar="P", help="add a permutation null of P relabellings")
    ap.add_argument("--residual-mode", choices=("moran", "geary"), default="moran")
    a = ap.parse_args(argv)
    if (a.residual_perms is not None or a.residual_mode != "moran") and not a.residual_autocorr:
        ap.error("--residual-perms and --residual-mode belong to --residual-autocorr")
    return a


def main():
    a = parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    sd_true = None
    if a.sparse_expression is not None:
        X, Y, Xv, Yv = sparse_expression_data(a, gen, dev)
    else:
        X, Y, sd_true = synthetic_expression(a.spots, a.genes, a.factors, gen)
        n_val = max(int(a.holdout * a.spots), 1)
        perm = torch.randperm(a.spots, generator=gen)
        held, fit = perm[:n_val], perm[n_val:]
        Xv, Yv, X, Y = X[held], Y[:, held], X[fit], Y[:, fit]
    print(f"{Y.shape[1]} spots to fit, {Yv.shape[1]} held out")

    L, M = a.factors, a.inducing
    kernel = NSF_RBF(sigma=1.0, lengthscale=30.0, L=L)
    gp = WSVGP(kernel, dim=2, M=M, jitter=1e-2)
    gp.Z = nn.Parameter(X[torch.randperm(X.shape[0], generator=gen)[:M]].clone().cpu(), requires_grad=False)
    gp.mu = nn.Parameter(1e-2 * torch.randn(L, M, generator=gen))
    gp.Lu = nn.Parameter(1e-2 * torch.randn(L, M, M, generator=gen) - 1.0 * torch.eye(M))
    kernel.sigma.requires_grad_(False); kernel.lengthscale.requires_grad_(False)
    model = RSF(gp, Y, L=L).to(dev)
    X, Y, Xv, Yv = X.to(dev), Y.to(dev), Xv.to(dev), Yv.to(dev)
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=a.lr)
    batch = min(a.batch, X.shape[0])

    before = model.score(Xv, Yv)
    train_batched(model, opt, X, Y, dev, steps=3, batch_size=batch)                          # warm-up (workspaces, caches)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = train_batched(model, opt, X, Y, dev, steps=a.steps, batch_size=batch)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    k = max(a.steps // 10, 1)
    print(f"N={X.shape[0]} spots, D={a.genes} genes, L={L} factors, M={M} inducing points, batch {batch}")
    print("loss (mean of first / last %d steps): %.1f -> %.1f" % (k, sum(losses[:k]) / k, sum(losses[-k:]) / k))
    print("%.1f ms per step (forward + backward + Adam), %.1f s for %d steps" % (1e3 * dt / a.steps, dt, a.steps))
    after = model.score(Xv, Yv)
    fit_sd = torch.nn.functional.softplus(model.noise.detach()).cpu()
    print("held-out spots:  R^2 %.3f -> %.3f, mse %.4f -> %.4f, expected loglik %.4g -> %.4g"
          % (float(before.r2), float(after.r2), float(before.mse), float(after.mse), float(before.loglik), float(after.loglik)))
    print("noise sd, median fitted %.3f%s; %d of %d loadings negative"
          % (float(fit_sd.median()), "" if sd_true is None else " (true %.3f)" % float(sd_true.median()),
             int((model.W < 0).sum()), model.W.numel()))
    assert sum(losses[-k:]) < sum(losses[:k]) and float(after.r2) > float(before.r2)
    if a.residual_autocorr:
        report_residual_autocorr(model, X, Y, a)


if __name__ == "__main__":
    main()
