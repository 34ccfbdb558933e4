"""Starting values of the NMF behind ``regularized_nmf``: sklearn's ``_initialize_nmf`` on torch tensors of any device.

'random' draws on the host from numpy's ``RandomState`` exactly as sklearn does.  The NNDSVD family is a deterministic
function of the leading L singular triplets of X (and does not depend on the signs of the singular vectors), so the
triplets need not come from sklearn's randomized SVD to give sklearn's starting values: they are computed here on the
tensor's device in fp64 by subspace iteration, and agree with sklearn's wherever both are converged (a clear gap after
the L-th singular value).  Nothing of size N or D travels to the host: the orthonormalisations are CholeskyQR2, whose
only host work is on (L+10) x (L+10) matrices, and no GPU solver library is involved.  The two large products per pass
(X Q and X^T Q) are ``torch.matmul``: this is a handful of iterations' worth of arithmetic, run once.

X may also be the transposed view of a ``likelihoods.SparseCounts`` (``counts.T``, obs x feat): the two large products then
go through ``ops.counts_matmul`` over the stored non-zeros and the mean is the fp64 sum of the stored values over N D;
everything else runs as for a dense X on the small dense factors.  No dense or ``torch.sparse`` form of X is made.
"""
from __future__ import annotations

import numpy as np
import torch

INITS = (None, "random", "nndsvd", "nndsvda", "nndsvdar")


def _orthonormalise(Y):
    """Columns of Y (n, k), k small, made orthonormal by CholeskyQR2: Y <- Y R^-1 with R^T R = Y^T Y, twice.  Only the
    (k, k) Gram matrix visits the host.  A Gram matrix that is not numerically positive definite (rank-deficient Y: X
    of rank below k) falls back to its eigen-decomposition and keeps the directions that carry something."""
    for _ in range(2):
        G = (Y.T @ Y).cpu().numpy()
        try:
            R = np.linalg.cholesky(G).T
            T = np.linalg.inv(R)
        except np.linalg.LinAlgError:
            lam, V = np.linalg.eigh(G)
            keep = lam > lam.max() * 1e-14 if lam.max() > 0 else np.zeros_like(lam, dtype=bool)
            T = V[:, keep] / np.sqrt(lam[keep])
        Y = Y @ torch.as_tensor(np.ascontiguousarray(T), dtype=Y.dtype, device=Y.device)
    return Y


def _is_counts(X):
    from .likelihoods import TransposedCounts
    return isinstance(X, TransposedCounts)


def _products(X):
    """(Q -> X Q, Q -> X^T Q, Y -> Y^T X) in fp64 for a dense tensor or a ``TransposedCounts``."""
    if _is_counts(X):
        from . import ops
        xtq = lambda Q: ops.counts_matmul(X, Q, transpose=True)
        return (lambda Q: ops.counts_matmul(X, Q)), xtq, (lambda Y: xtq(Y).T)
    A = X.to(torch.float64)
    return (lambda Q: A @ Q), (lambda Q: A.T @ Q), (lambda Y: Y.T @ A)


def leading_triplets(X, L, random_state=None, n_oversamples=10):
    """(U (N,L), S (L,), V (L,D)) fp64 on X's device: the L leading singular triplets of X by subspace iteration with
    sklearn's sizes (L + 10 columns; 7 passes when L < 0.1 min(N, D), else 4) from
    ``RandomState(random_state).normal(size=(D, L + 10))``.  X: a dense tensor or a ``TransposedCounts``."""
    xq, xtq, ytx = _products(X)
    N, D = X.shape
    device = X.device
    k = L + n_oversamples
    passes = 7 if L < 0.1 * min(N, D) else 4
    rng = np.random.RandomState(random_state) if not isinstance(random_state, np.random.RandomState) else random_state
    Q = torch.as_tensor(rng.normal(size=(D, k)), dtype=torch.float64, device=device)
    for _ in range(passes):
        Q = _orthonormalise(xq(Q))           # (N, k)
        Q = _orthonormalise(xtq(Q))          # (D, k)
    Y = _orthonormalise(xq(Q))               # (N, k') orthonormal basis of the leading left subspace
    B = ytx(Y)                               # (k', D)
    lam, E = np.linalg.eigh((B @ B.T).cpu().numpy())
    order = np.argsort(-lam)[:L]
    S = np.sqrt(np.clip(lam[order], 0.0, None))
    E = torch.as_tensor(np.ascontiguousarray(E[:, order]), dtype=torch.float64, device=device)    # (k', <=L)
    S_dev = torch.as_tensor(S, dtype=torch.float64, device=device)
    U = Y @ E
    V = (E.T @ B) / torch.where(S_dev > 0, S_dev, torch.ones_like(S_dev)).unsqueeze(1)
    if U.shape[1] < L:                       # X of rank below L: the missing triplets are zero
        U = torch.cat([U, U.new_zeros(N, L - U.shape[1])], 1)
        V = torch.cat([V, V.new_zeros(L - V.shape[0], D)], 0)
        S_dev = torch.cat([S_dev, S_dev.new_zeros(L - S_dev.shape[0])])
    return U, S_dev, V


def _fill_zeros(M, values_for):
    zero = M == 0
    nz = int(zero.sum())                     # the one count that comes back to the host
    if nz:
        M[zero] = torch.as_tensor(values_for(nz), dtype=M.dtype, device=M.device)    # row-major order, as numpy's


def initialize_nmf(X, L, init=None, random_state=None, eps=1e-6):
    """Starting ``(W0 (N,L), H0 (L,D))`` of an NMF of X (N,D) >= 0 (a float tensor on any device, or ``counts.T`` of a
    ``SparseCounts``, on a CUDA device for the NNDSVD family), of X's dtype and on X's device, following sklearn's
    ``_initialize_nmf``: ``init`` one of 'random', 'nndsvd', 'nndsvda', 'nndsvdar' or
    None (= 'nndsvda' when L <= min(N, D), else 'random').  'random' and the random fill of 'nndsvdar' use numpy's
    ``RandomState(random_state)`` draw for draw like sklearn (H before W for 'random'; W's zeros in row-major order, then
    H's, from a fresh generator for the fill), so they reproduce sklearn's values wherever the zero patterns agree."""
    if init not in INITS:
        raise ValueError(f"initialize_nmf: init={init!r} unsupported (one of {INITS})")
    counts = _is_counts(X)
    if not counts and (not isinstance(X, torch.Tensor) or X.dim() != 2 or not X.is_floating_point()):
        raise ValueError("initialize_nmf: X must be a 2-D floating-point tensor or the .T of a SparseCounts")
    N, D = X.shape
    L = int(L)
    if L < 1:
        raise ValueError(f"initialize_nmf: L={L} unsupported (>= 1)")
    if init not in (None, "random") and L > min(N, D):
        raise ValueError(f"init = '{init}' can only be used when n_components <= min(n_samples, n_features)")
    if init is None:
        init = "nndsvda" if L <= min(N, D) else "random"
    np_dtype = np.float32 if X.dtype == torch.float32 else np.float64
    mean = float(X.T.col_val.sum(dtype=torch.float64)) / (N * D) if counts else float(X.to(torch.float64).mean())

    if init == "random":
        avg = np.sqrt(np_dtype(mean) / L) if np_dtype is np.float32 else np.sqrt(mean / L)
        rng = np.random.RandomState(random_state) if not isinstance(random_state, np.random.RandomState) else random_state
        H = avg * rng.standard_normal(size=(L, D)).astype(np_dtype, copy=False)
        W = avg * rng.standard_normal(size=(N, L)).astype(np_dtype, copy=False)
        np.abs(H, out=H)
        np.abs(W, out=W)
        return (torch.as_tensor(W, dtype=X.dtype, device=X.device), torch.as_tensor(H, dtype=X.dtype, device=X.device))

    U, S, V = leading_triplets(X, L, random_state=random_state)
    W = torch.zeros_like(U)
    H = torch.zeros_like(V)
    root = torch.sqrt(S)
    W[:, 0] = root[0] * U[:, 0].abs()
    H[0, :] = root[0] * V[0, :].abs()
    if L > 1:
        # the positive and negative parts of every further pair and their norms, all pairs at once
        Up, Un, Vp, Vn = U[:, 1:].clamp(min=0), (-U[:, 1:]).clamp(min=0), V[1:].clamp(min=0), (-V[1:]).clamp(min=0)
        up, un, vp, vn = Up.norm(dim=0), Un.norm(dim=0), Vp.norm(dim=1), Vn.norm(dim=1)
        m_p, m_n = up * vp, un * vn
        pos = m_p > m_n
        one = torch.ones_like(up)
        u = torch.where(pos, Up / torch.where(up > 0, up, one), Un / torch.where(un > 0, un, one))
        v = torch.where(pos.unsqueeze(1), Vp / torch.where(vp > 0, vp, one).unsqueeze(1),
                        Vn / torch.where(vn > 0, vn, one).unsqueeze(1))
        lbd = torch.sqrt(S[1:] * torch.where(pos, m_p, m_n))
        W[:, 1:] = u * lbd
        H[1:] = v * lbd.unsqueeze(1)
    W[W < eps] = 0
    H[H < eps] = 0
    if init == "nndsvda":
        W[W == 0] = mean
        H[H == 0] = mean
    elif init == "nndsvdar":
        rng = np.random.RandomState(random_state) if not isinstance(random_state, np.random.RandomState) else random_state
        _fill_zeros(W, lambda n: np.abs(mean * rng.standard_normal(size=n) / 100))
        _fill_zeros(H, lambda n: np.abs(mean * rng.standard_normal(size=n) / 100))
    return W.to(X.dtype).contiguous(), H.to(X.dtype).contiguous()
