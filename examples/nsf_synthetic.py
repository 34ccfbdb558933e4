#!/usr/bin/env python3
"""Non-negative spatial factorisation on synthetic Slide-seq-shaped counts, written the way the reference's
notebooks are (Slideseq_NSF_newest_version.ipynb): NSF_RBF kernel, SVGP prior with inducing points drawn
from the spots, NSF2 likelihood, kernel hyper-parameters frozen, `train_batched` over mini-batches of spots.

    PYTHONPATH=. python examples/nsf_synthetic.py [--spots 40000 --genes 2000 --factors 10 --inducing 2000 --steps 200]

``--sparse-counts DENSITY`` thins the counts to that fraction of non-zeros (real Slide-seq / Visium matrices are a few per
cent dense) and fits through ``SparseCounts``: the same model and the same loop, the step over the non-zeros only (under
``--likelihood nb`` plus a dense pass over the batch that reads no counts).

``--holdout FRAC`` holds that fraction of the spots out (``train_val_split``, the split of the reference's
``anndata_to_train_val``), fits on the rest and prints the Poisson deviance of the held-out spots under the predictive mean
rate and the share of the null model's deviance it explains (``model.deviance``); it works with ``--sparse-counts`` too.  With ``--residual-autocorr`` it prints the ten genes with the largest
``z`` of ``model.residual_autocorr`` after the fit: where spatial structure is left in what the model did not explain;
``--residual-perms P`` (with ``--residual-mode geary`` for Geary's C) adds the permutation null and prints the ten genes
with the smallest permutation p-value for positive autocorrelation and their Benjamini-Hochberg value (``fdr_bh``).

``--likelihood nb`` draws overdispersed (gamma-Poisson) counts with a known inverse dispersion per gene, fits the model with
``likelihood="nb"`` (the fused negative-binomial step) and prints the fitted theta next to the true one; with ``--holdout``
it also prints the held-out NB deviance, the fraction of the NB null deviance it explains and ``loglik - poisson_loglik``,
what the dispersion parameter earned on the held-out spots (``model.deviance(..., family="nb")``).  With
``--sparse-counts`` the thinned counts are no longer gamma-Poisson with the true theta, so the two columns need not agree.
``--theta0 mle`` (with ``--sparse-counts``) first fits every gene's theta by maximum likelihood under the constant-rate null
(``gene_dispersion``), prints the share of genes with ``pvalue < 0.01`` and the median of that theta against the true one,
and starts the model's theta there instead of at 10.
"""
import argparse
import math
import time

import torch
import torch.nn as nn

from gpzoo.gp import SVGP
from gpzoo.kernels import NSF_RBF
from gpzoo.likelihoods import NSF2, SparseCounts
from gpzoo.utilities import gene_dispersion, init_softplus, train_batched, train_val_split


def synthetic_counts(N, D, L, gen, theta=None):
    """Smooth non-negative spatial factors on a 2-D tissue, gene loadings and Poisson counts -- gamma-Poisson ones with
    inverse dispersion ``theta`` (D,) per gene when given (mean as before, variance mean + mean^2 / theta)."""
    X = (torch.rand(N, 2, generator=gen) - 0.5) * 200.0
    centres = (torch.rand(L, 2, generator=gen) - 0.5) * 160.0
    F = torch.exp(-((X[None] - centres[:, None]) ** 2).sum(-1) / (2 * 35.0 ** 2))          # (L,N)
    W = torch.rand(D, L, generator=gen) ** 3 * 4.0
    rate = W @ F + 0.05
    if theta is not None:
        torch.manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=gen)))        # Gamma.sample takes no generator
        rate = torch.distributions.Gamma(theta[:, None].expand_as(rate), theta[:, None] / rate).sample()
    Y = torch.poisson(rate, generator=gen)
    return X, Y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spots", type=int, default=40000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--factors", type=int, default=10)
    ap.add_argument("--inducing", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=7000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--sparse-counts", type=float, default=None, metavar="DENSITY",
                    help="keep about this fraction of the counts as non-zeros and fit through SparseCounts")
    ap.add_argument("--lr", type=float, default=1e-2, help="Adam's learning rate")
    ap.add_argument("--holdout", type=float, default=None, metavar="FRAC",
                    help="hold this fraction of the spots out and print their deviance under the fitted model")
    ap.add_argument("--likelihood", choices=["poisson", "nb"], default="poisson",
                    help="nb: gamma-Poisson counts and the negative-binomial model with one inverse dispersion per gene")
    ap.add_argument("--theta0", default="10", metavar="VALUE|mle",
                    help="nb: where every gene's theta starts; mle: each gene's own maximum-likelihood theta under the "
                         "constant-rate null (gene_dispersion; needs --sparse-counts)")
    ap.add_argument("--residual-autocorr", action="store_true",
                    help="after the fit, print the ten genes whose residuals are most spatially autocorrelated")
    ap.add_argument("--residual-perms", type=int, default=None, metavar="P",
                    help="with --residual-autocorr: P random relabellings of the spots; print the ten genes with the smallest "
                         "permutation p-value and their fdr_bh value")
    ap.add_argument("--residual-mode", default="moran", choices=("moran", "geary"), help="with --residual-perms: the statistic")
    a = ap.parse_args()
    if a.residual_perms is not None and not a.residual_autocorr:
        ap.error("--residual-perms needs --residual-autocorr")
    if a.theta0 == "mle" and (a.likelihood != "nb" or a.sparse_counts is None):
        ap.error("--theta0 mle needs --likelihood nb and --sparse-counts (gene_dispersion reads a SparseCounts)")
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    theta_true = None
    if a.likelihood == "nb":
        theta_true = torch.exp(math.log(0.5) + (math.log(20.0) - math.log(0.5)) * torch.rand(a.genes, generator=gen))
    X, Y = synthetic_counts(a.spots, a.genes, a.factors, gen, theta_true)
    L, M = a.factors, a.inducing
    if a.sparse_counts is not None:
        Y = Y * (torch.rand(Y.shape, generator=gen) < a.sparse_counts)
        dense_bytes = Y.numel() * 4
        Y = SparseCounts(Y)
        held = sum(getattr(Y, k).numel() * getattr(Y, k).element_size() for k in Y._PARTS)
        print(f"{Y.nnz} non-zeros ({100.0 * Y.nnz / (a.spots * a.genes):.1f} %): {held / 2 ** 20:.1f} MiB held in both orders, "
              f"{dense_bytes / 2 ** 20:.1f} MiB as a dense fp32 array")

    val = None
    if a.holdout is not None:
        # the spots are drawn independently, so the first ones are a random subset; size factors per split as scanpy's
        tr, val = train_val_split(X, Y, train_frac=1.0 - a.holdout, sz="scanpy")
        if val is None:
            raise SystemExit(f"--holdout {a.holdout} holds no spot out of {a.spots}")
        X, Y = tr["X"], tr["y"]
        print(f"{Y.shape[1]} spots to fit, {val['y'].shape[1]} held out")

    kernel = NSF_RBF(sigma=1.0, lengthscale=20.0, L=L)
    gp = SVGP(kernel, dim=2, M=M, jitter=1e-1)
    gp.Z = nn.Parameter(X[torch.randperm(X.shape[0], generator=gen)[:M]].clone(), requires_grad=False)
    gp.mu = nn.Parameter(torch.zeros(L, M))
    gp.Lu = nn.Parameter(1e-2 * torch.randn(L, M, M, generator=gen))
    kernel.sigma.requires_grad_(False); kernel.lengthscale.requires_grad_(False)   # as in the notebooks
    theta0 = 10.0 if a.theta0 == "mle" else float(a.theta0)
    if a.theta0 == "mle":
        # which genes are overdispersed at all, and a start per gene: the null holds each gene's rate constant, so its theta
        # absorbs the variation the factors will explain -- a lower-biased start, not an estimate of the model's theta
        disp = gene_dispersion(Y.to(dev))
        found = torch.isfinite(disp.theta)
        print("gene-wise NB fit under the constant-rate null: %.1f %% of the genes overdispersed at p < 0.01; median theta %.2f "
              "(true %.2f)" % (100.0 * float((disp.pvalue < 0.01).double().mean()), float(disp.theta[found].median()),
                               float(theta_true.median())))
        theta0 = disp.theta.nan_to_num(nan=10.0).clamp(1e-2, 1e3).cpu()
    model = NSF2(gp, Y, L=L, likelihood=a.likelihood, theta0=theta0)
    if val is not None:
        # size factors as fixed offsets (each spot's depth over the median): the held-out spots then have theirs too
        model.V = nn.Parameter(torch.from_numpy(init_softplus(tr["sz"].clamp_min(1e-3).numpy())), requires_grad=False)
        # ... and the factors start at the level of the data: V softplus(W) exp(mu) summed over L factors ~ the mean count
        level = float(Y.col_val.sum() / (Y.shape[0] * Y.shape[1]) if isinstance(Y, SparseCounts) else Y.mean())
        gp.mu.data.fill_(math.log(max(level, 1e-6) / L))
    model = model.to(dev)
    X, Y = X.to(dev), Y.to(dev)
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=a.lr)

    train_batched(model, opt, X, Y, dev, steps=3, E=a.samples, batch_size=a.batch)          # warm-up (workspaces, caches)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = train_batched(model, opt, X, Y, dev, steps=a.steps, E=a.samples, batch_size=a.batch)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    k = max(a.steps // 10, 1)
    print(f"N={X.shape[0]} spots, D={a.genes} genes, L={L} factors, M={M} inducing points, batch {a.batch}, E={a.samples}")
    print("loss (mean of first / last %d steps): %.1f -> %.1f" % (k, sum(losses[:k]) / k, sum(losses[-k:]) / k))
    print("%.1f ms per step (forward + backward + Adam), %.1f s for %d steps" % (1e3 * dt / a.steps, dt, a.steps))
    assert sum(losses[-k:]) < sum(losses[:k])
    if theta_true is not None:
        fit_theta = torch.nn.functional.softplus(model.theta.detach()).cpu()
        order = torch.argsort(theta_true)
        pick = order[torch.linspace(0, a.genes - 1, min(8, a.genes)).long()]
        print("theta (true -> fitted, genes across the range): " + ", ".join(f"{float(theta_true[i]):.2f} -> {float(fit_theta[i]):.2f}" for i in pick))
        lt, lf = torch.log(theta_true), torch.log(fit_theta)
        print("median fitted theta %.2f (true %.2f, start %s); correlation of log theta %.2f"
              % (float(fit_theta.median()), float(theta_true.median()), "the gene-wise fit" if a.theta0 == "mle" else a.theta0,
                 float(torch.corrcoef(torch.stack([lt, lf]))[0, 1])))
    if val is not None:
        fit = model.deviance(X, Y)
        V_val = val["sz"].to(dev).clamp_min(1e-3)
        t0 = time.perf_counter()
        r = model.deviance(val["X"].to(dev), val["y"].to(dev), V=V_val)
        total, explained = float(r.total), float(r.explained)                              # waits for the device
        dt = time.perf_counter() - t0
        print("training spots:  deviance %.4g (%.4f per entry), explained %.3f" % (float(fit.total), float(fit.mean), float(fit.explained)))
        print("held-out spots:  deviance %.4g (%.4f per entry), explained %.3f, sum mu / sum y %.3f  [%.1f ms]"
              % (total, float(r.mean), explained, float(r.sum_mu / r.sum_y), 1e3 * dt))
        assert total == total and abs(total) != float("inf") and 0.0 < explained < 1.0
        if a.likelihood == "nb":
            # the same spots under the model's own likelihood: the NB deviance with the fitted theta, and what theta earned
            # over Poisson noise at the same rate, in log density (deviances of different families are not comparable)
            nb = model.deviance(val["X"].to(dev), val["y"].to(dev), V=V_val, family="nb")
            gain = nb.loglik_per_gene - nb.poisson_loglik_per_gene
            print("held-out spots:  NB deviance %.4g (%.4f per entry), explained %.3f, loglik - poisson_loglik %.4g "
                  "(%d of %d genes gain)" % (float(nb.total), float(nb.mean), float(nb.explained),
                                             float(nb.loglik - nb.poisson_loglik), int((gain > 0).sum()), gain.numel()))
            assert float(nb.total) == float(nb.total) and abs(float(nb.loglik)) != float("inf")
    if a.residual_autocorr:
        # is spatial structure left in what the fit did not explain, and in which genes: Moran's I of each gene's Pearson
        # residuals over the fitted spots' 6-nearest-neighbour graph (z ranks genes; it is not a calibrated test)
        t0 = time.perf_counter()
        ra = model.residual_autocorr(X, Y)
        top = torch.argsort(ra.z, descending=True)[:10].cpu()
        dt = time.perf_counter() - t0
        print("residual autocorrelation (Pearson, family %s) of %d genes over %d spots  [%.1f ms]; expected I %.2e, sd %.2e"
              % (a.likelihood, a.genes, X.shape[0], 1e3 * dt, float(ra.expected), float(ra.variance.sqrt())))
        for i in top.tolist():
            print("  gene %5d  I %+.4f  z %+7.2f  residual mean %+.3f  variance %.3f"
                  % (i, float(ra.I[i]), float(ra.z[i]), float(ra.residual_mean[i]), float(ra.residual_var[i])))
        assert bool(torch.isfinite(ra.I).all())
        if a.residual_perms is not None:
            # how unusual each gene's statistic is among relabellings of its own residuals: exact for exchangeable residuals,
            # still blind to the degrees of freedom the fit used
            from gpzoo.utilities import fdr_bh
            t0 = time.perf_counter()
            rp = model.residual_autocorr(X, Y, mode=a.residual_mode, assumption="randomisation", n_perms=a.residual_perms, seed=0)
            geary = a.residual_mode == "geary"
            pval = rp.pval_less if geary else rp.pval_greater          # positive autocorrelation: a small C, a large I
            q = fdr_bh(pval)
            top = torch.argsort(pval, stable=True)[:10].cpu()
            dt = time.perf_counter() - t0
            print("permutation null of %s over %d relabellings  [%.1f ms]; smallest attainable p %.4f"
                  % ("Geary's C" if geary else "Moran's I", rp.n_perms, 1e3 * dt, 1.0 / (rp.n_perms + 1)))
            for i in top.tolist():
                print("  gene %5d  %s %+.4f  p %.4f  fdr_bh %.4f  z (randomisation) %+7.2f  residual kurtosis %.1f"
                      % (i, "C" if geary else "I", float(rp[0][i]), float(pval[i]), float(q[i]), float(rp.z[i]),
                         float(rp.residual_kurtosis[i])))
            assert bool(((pval > 0) & (pval <= 1)).all())


if __name__ == "__main__":
    main()
