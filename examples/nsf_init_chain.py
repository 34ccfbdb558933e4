#!/usr/bin/env python3
"""The NSF notebooks' initialisation chain, every step of it on this package (no sklearn, anndata or squidpy):

    rescale_spatial_coords -> regularized_nmf -> inducing points -> smooth_spatial_factors -> gp.mu, model.W -> train

on synthetic counts, against the same model started from mu = 0 and random loadings.

    PYTHONPATH=. python examples/nsf_init_chain.py [--spots 20000 --genes 500 --factors 6 --inducing 500 --steps 30
                                                   --inducing-from {subset,kmeans} --mu-from {smooth,projection}
                                                   --sparse-counts DENSITY [--select-genes NFEAT --rank-by {deviance,moran,geary,gp}]
                                                   [--moran-perms P]]

``--sparse-counts DENSITY`` thins the counts to about that fraction of non-zeros and runs the whole chain on them as a
``SparseCounts``: the size factors and the NMF start from ``counts.T``, the fit from ``counts``.  The dense count array
then never reaches the device.  ``--select-genes NFEAT`` ranks the genes of those counts first (``rank_genes``: Poisson deviance
against a constant-rate null, Moran's I / 1 - Geary's C of the log-normalised counts over the spots' 6-neighbour graph, or the
sparse-GP likelihood ratio of ``gene_spatial_gp``, which also prints the median length scale it selects beside the one the
model's kernel starts from) and runs the chain
on the NFEAT best (``counts.select_genes``) -- the reference's ``ad[:, :nfeat]`` of genes sorted by importance.  The size
factors stay those of the whole data set.  ``--moran-perms P`` then scores the genes that are left with Moran's I under P
random relabellings of the spots (``gene_autocorr(..., n_perms=P)``) and prints how many have a Benjamini-Hochberg adjusted
pseudo p-value below 0.05 (with P permutations no p-value is below 1 / (P + 1): a few hundred are needed for that).
"""
import argparse

import numpy as np
import torch
import torch.nn as nn

from gpzoo.gp import SVGP
from gpzoo.kernels import NSF_RBF
from gpzoo.likelihoods import NSF2, SparseCounts
from gpzoo.utilities import (fdr_bh, gene_autocorr, gene_spatial_gp, init_softplus, kmeans_inducing_points, log_normalize,
                             project_factors_to_inducing, regularized_nmf, rank_genes, rescale_spatial_coords, scanpy_sizefactors,
                             smooth_spatial_factors, train)


def synthetic_counts(N, D, L, rng):
    X = (rng.random((N, 2)) * np.array([[6400.0, 3100.0]]) + 500.0).astype(np.float32)          # pixel coordinates
    centres = X[rng.choice(N, L, replace=False)]
    F = np.exp(-((X[None] - centres[:, None]) ** 2).sum(-1) / (2 * 700.0 ** 2))                  # (L,N)
    W = rng.random((D, L)) ** 3 * 4.0
    return X, rng.poisson(W @ F + 0.05).T.astype(np.float32)                                     # Y (N,D)


def model_for(X, Y, Z, L, dev, mu=None, W=None):
    kernel = NSF_RBF(sigma=1.0, lengthscale=0.4, L=L)
    gp = SVGP(kernel, dim=2, M=len(Z), jitter=1e-2)
    gp.Z = nn.Parameter(torch.as_tensor(Z), requires_grad=False)
    gp.mu = nn.Parameter(torch.zeros(L, len(Z)) if mu is None else torch.as_tensor(mu, dtype=torch.float32))
    gp.Lu = nn.Parameter(1e-2 * torch.eye(len(Z)).repeat(L, 1, 1))
    kernel.sigma.requires_grad_(False); kernel.lengthscale.requires_grad_(False)                 # as in the notebooks
    model = NSF2(gp, Y if isinstance(Y, SparseCounts) else torch.as_tensor(Y.T), L=L)       # only the shape (D, N) is read
    if W is not None:
        model.W = nn.Parameter(torch.as_tensor(init_softplus(W), dtype=torch.float32))           # softplus(model.W) = W
    return model.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spots", type=int, default=20000)
    ap.add_argument("--genes", type=int, default=500)
    ap.add_argument("--factors", type=int, default=6)
    ap.add_argument("--inducing", type=int, default=500)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--inducing-from", "--inducing_from", choices=("subset", "kmeans"), default="subset",
                    help="inducing points: a random subset of the spots, or their k-means centres (kmeans_inducing_points)")
    ap.add_argument("--mu-from", "--mu_from", choices=("smooth", "projection"), default="smooth",
                    help="gp.mu: the kNN mean of the factors at Z (smooth_spatial_factors), or their kernel least-squares "
                         "projection onto Z (project_factors_to_inducing, the notebooks' Kzx @ Kxz composition)")
    ap.add_argument("--sparse-counts", type=float, default=None, metavar="DENSITY",
                    help="keep about this fraction of the counts as non-zeros and run the chain through SparseCounts")
    ap.add_argument("--select-genes", "--select_genes", type=int, default=None, metavar="NFEAT",
                    help="with --sparse-counts: rank the genes and keep the NFEAT best before the NMF start")
    ap.add_argument("--rank-by", "--rank_by", choices=("deviance", "moran", "geary", "gp"), default="deviance",
                    help="the score --select-genes ranks by (rank_genes)")
    ap.add_argument("--moran-perms", "--moran_perms", type=int, default=None, metavar="P",
                    help="with --sparse-counts: Moran's I of the genes under P relabellings of the spots, and how many genes "
                         "have fdr_bh(pval_sim) < 0.05")
    a = ap.parse_args()
    if a.select_genes is not None and a.sparse_counts is None:
        raise SystemExit("--select-genes ranks the stored non-zeros of a SparseCounts: pass --sparse-counts DENSITY with it")
    if a.moran_perms is not None and a.sparse_counts is None:
        raise SystemExit("--moran-perms scores the stored non-zeros of a SparseCounts: pass --sparse-counts DENSITY with it")
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    X, Y = synthetic_counts(a.spots, a.genes, a.factors, rng)
    L, M = a.factors, a.inducing
    nmf_kw = dict(solver="mu", init="nndsvdar", beta_loss="kullback-leibler", max_iter=200, random_state=0)

    X = rescale_spatial_coords(X)                                                                # roughly (-2, 2)
    if a.sparse_counts is not None:
        Y = Y * (rng.random(Y.shape) < a.sparse_counts)
        Y = SparseCounts(torch.as_tensor(Y.T)).to(dev)                                           # (D, N), non-zeros only
        print(f"sparse counts: {Y.nnz} non-zeros, {Y.nnz / (a.spots * a.genes):.1%} of {a.genes} x {a.spots}")
        sz = scanpy_sizefactors(Y.T)
        sz = np.maximum(sz, sz[sz > 0].min())           # a spot thinned to nothing says nothing about its depth; log(sz) stays finite
        if a.select_genes is not None:
            order, score = rank_genes(Y, by=a.rank_by, coords=X if a.rank_by in ("moran", "geary", "gp") else None, nfeat=a.select_genes)
            Y = Y.select_genes(order)
            if a.rank_by == "gp":
                fit = gene_spatial_gp(log_normalize(Y), X, inducing=min(256, a.spots))
                print(f"sparse-GP length scale of the selected genes: median {float(fit.lengthscale.nanmedian()):.3g} (grid "
                      f"{float(fit.lengthscales[0]):.3g} .. {float(fit.lengthscales[-1]):.3g}), median fraction of spatial variance "
                      f"{float(fit.fsv.nanmedian()):.3g}; the model's kernel starts at lengthscale 0.4")
            print(f"selected {Y.shape[0]} of {a.genes} genes by {a.rank_by}: score {float(score[0]):.4g} ... {float(score[-1]):.4g}, "
                  f"{Y.nnz} non-zeros kept")
        if a.moran_perms is not None:
            ac = gene_autocorr(log_normalize(Y, center=False), X, n_perms=a.moran_perms)
            q = fdr_bh(ac.pval_sim)
            print(f"Moran's I under {ac.n_perms} relabellings of the spots: {int((q < 0.05).sum())} of {Y.shape[0]} genes with "
                  f"fdr_bh(pval_sim) < 0.05 (smallest attainable p {1 / (ac.n_perms + 1):.3g}), median z_sim "
                  f"{float(ac.z_sim.nanmedian()):.3g}")
        F, W = regularized_nmf(Y.T, L, sz=sz, **nmf_kw)
    else:
        sz = scanpy_sizefactors(Y)
        F, W = regularized_nmf(torch.as_tensor(Y, device=dev), L, sz=sz, **nmf_kw)
    if a.inducing_from == "kmeans":
        Z = kmeans_inducing_points(X, M, random_state=0)
    else:
        Z = X[rng.choice(a.spots, M, replace=False)]
    U, beta0, beta = smooth_spatial_factors(F, Z, X)
    print(f"N={a.spots} D={a.genes} L={L} M={M}: F {F.shape} {F.dtype}, U {U.shape} {U.dtype}, trend {beta.shape}")
    start = "NMF + smooth_spatial_factors"
    if a.mu_from == "projection":
        # the model's kernel; SVGP: un-whitened.  float64 coordinates select the fp64 Gram pass: inducing points drawn from
        # the spots with a lengthscale above their spacing make K_zx K_xz nearly singular, and fp32 entries would move it
        # by more than the 1e-5 jitter
        mu, info = project_factors_to_inducing(NSF_RBF(sigma=1.0, lengthscale=0.4, L=L), np.asarray(Z, dtype=np.float64),
                                               X.astype(np.float64), np.ascontiguousarray(F.T), return_info=True)
        U, start = mu.T, "NMF + project_factors_to_inducing"
        print(f"  projection: residual per factor {np.array2string(info['residual'], precision=3)}, "
              f"diag(G) in [{info['gram_diag_min']:.3g}, {info['gram_diag_max']:.3g}]")

    Xd = torch.as_tensor(X, device=dev)
    Yd = Y if isinstance(Y, SparseCounts) else torch.as_tensor(Y.T, device=dev)
    for name, model in ((start, model_for(X, Y, Z, L, dev, mu=U.T, W=W)),
                        ("mu = 0, random loadings", model_for(X, Y, Z, L, dev))):
        with torch.no_grad():
            model.V.copy_(torch.as_tensor(init_softplus(sz[:, 0].astype(np.float64))))
        opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-2)
        losses = train(model, opt, Xd, Yd, dev, steps=a.steps, E=3)
        print(f"  {name:34s} loss {losses[0]:.4g} -> {losses[-1]:.4g}")


if __name__ == "__main__":
    main()
