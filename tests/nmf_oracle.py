"""numpy oracle of the KL multiplicative-update NMF behind regularized_nmf: the iteration, the stopping rule, the
divergence and the post-processing.  Imports neither sklearn nor the reference.

Written operation for operation like sklearn 1.7's ``_fit_multiplicative_update`` for ``beta_loss = 1`` without
regularisation (``_multiplicative_update_w``, ``_multiplicative_update_h``, ``_beta_divergence``): in fp64 it gives
sklearn's W, H and n_iter bit for bit (tests/test_nmf.py checks that where sklearn is installed).  EPS is the float32
epsilon whatever the dtype, as in sklearn."""
from __future__ import annotations

import numpy as np

EPS = np.finfo(np.float32).eps


def planted_counts(N, D, L, seed):
    """The issue's planted count matrix: Y = Poisson(6 F W / L), F ~ Gamma(0.6) (N,L), W ~ Gamma(0.5) (L,D)."""
    rng = np.random.default_rng(seed)
    F = rng.gamma(0.6, size=(N, L))
    W = rng.gamma(0.5, size=(L, D))
    return rng.poisson(6.0 * (F @ W) / L).astype(np.float64)


def kl_divergence(X, W, H):
    """sqrt(2 * generalised KL(X || W H)) as ``_beta_divergence(X, W, H, 1, square_root=True)`` forms it."""
    X, W, H = np.atleast_2d(X), np.atleast_2d(W), np.atleast_2d(H)
    WH_data = np.dot(W, H).ravel()
    X_data = X.ravel()
    keep = X_data > EPS
    WH_data = WH_data[keep]
    X_data = X_data[keep]
    WH_data[WH_data < EPS] = EPS
    sum_WH = np.dot(np.sum(W, axis=0), np.sum(H, axis=1))
    res = np.dot(X_data, np.log(X_data / WH_data))
    res += sum_WH - X_data.sum()
    return np.sqrt(2 * max(res, 0))


def update_w(X, W, H):
    Q = np.dot(W, H)
    Q[Q < EPS] = EPS
    np.divide(X, Q, out=Q)
    numerator = np.dot(Q, H.T)
    denominator = np.sum(H, axis=1)[np.newaxis, :]
    denominator[denominator == 0] = EPS
    numerator /= denominator
    W *= numerator
    return W


def update_h(X, W, H):
    Q = np.dot(W, H)
    Q[Q < EPS] = EPS
    np.divide(X, Q, out=Q)
    numerator = np.dot(W.T, Q)
    W_sum = np.sum(W, axis=0)
    W_sum[W_sum == 0] = 1.0
    denominator = W_sum[:, np.newaxis]
    numerator /= denominator
    H *= numerator
    H[H < np.finfo(np.float64).eps] = 0.0
    return H


def fit_mu(X, W0, H0, max_iter=200, tol=1e-4):
    """(W, H, n_iter): the divergence before the loop, W then H every iteration, the divergence again after every 10th
    iteration when tol > 0, stopping when (previous - error) / error_at_init < tol."""
    W, H = np.array(W0, copy=True), np.array(H0, copy=True)
    error_at_init = kl_divergence(X, W, H)
    previous_error = error_at_init
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        W = update_w(X, W, H)
        H = update_h(X, W, H)
        if tol > 0 and n_iter % 10 == 0:
            error = kl_divergence(X, W, H)
            if (previous_error - error) / error_at_init < tol:
                break
            previous_error = error
    return W, H, n_iter


def postprocess(eF, Wl, L, sz=1, pseudocount=1e-2, shrinkage=0.2):
    """(F (N,L), W (D,L)) from NMF factors eF (N,L) and loadings Wl (D,L): shrink both towards their means (sums kept),
    log scale, recentre the factors to the lognormal prior mean, fold shift and 1 / colsum into the loadings."""
    a = shrinkage
    W = np.asarray(Wl)
    if 0 < a < 1:
        W = W * (1 - a) + a * W.sum(axis=0) / float(W.shape[0])
    wsum = W.sum(axis=0)
    eF = np.asarray(eF) * wsum
    if 0 < a < 1:
        eF = eF * (1 - a) + a * eF.sum(axis=1, keepdims=True) / float(eF.shape[1])
    F = np.log(pseudocount + eF) - np.log(sz)
    Lp = max(L, 1.1)
    sigma2 = np.log(2 * Lp) - np.log(Lp + 1)
    mu = -np.log(Lp) - sigma2 / 2.0
    shift = F.mean(axis=0) - mu
    return F - shift, W * np.exp(shift - np.log(wsum))
