"""Numeric helpers importable under the reference's names (gpzoo/utilities.py).

On the fused HIP path none of these is called: jitter, the whitened KL and the
svgp_forward moments are produced inside ``gpz_svgp_forward``.  They exist so
notebook code that calls them directly on its own tensors keeps working; they
are element-wise / tiny operations expressed with torch on whatever device the
caller's tensors live on.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch


def _torch_sqrt(x, eps=1e-12):
    """sqrt(x + eps): avoids the NaN gradient of sqrt at 0 (reference utilities.py:450-456)."""
    return (x + eps).sqrt()


def _embed_distance_matrix(distance_matrix):
    """Classical-MDS embedding of a (G,G) group-distance matrix (reference
    utilities.py:459-469).  G is a handful of tissue groups: stays in torch, runs once."""
    G = len(distance_matrix)
    centre = torch.eye(G) - torch.full((G, G), 1.0 / G)
    gram = -0.5 * (centre @ (distance_matrix ** 2) @ centre)
    evals, evecs = torch.linalg.eigh(gram)
    evals = evals.clamp(min=0)
    return evecs @ torch.diag(_torch_sqrt(evals, 1e-6))


def _squared_dist(X, Z):
    """Pairwise squared distances, clamped at zero (reference utilities.py:399-405)."""
    r2 = (X ** 2).sum(1, keepdim=True) - 2 * X.matmul(Z.t()) + (Z ** 2).sum(1, keepdim=True).t()
    return r2.clamp(min=0)


def add_jitter(K, jitter=1e-3):
    """IN-PLACE diagonal jitter on (M,M) or (L,M,M); returns the same tensor, and
    None for other ranks like the reference (utilities.py:407-418)."""
    if K.dim() in (2, 3):
        K.diagonal(dim1=-2, dim2=-1).add_(jitter)
        return K
    return None


def reshape_param(param):
    return param.view(-1, param.shape[-2], param.shape[-1])


def whitened_KL(mz, Lz):
    """KL(N(mz, Lz Lz^T) || N(0, I)) for ONE GP: mz (M,), Lz (M,M) -- the reference's
    2-D-only contract (utilities.py:27-36).  Use ``whitened_KL_batched`` for (L,M,M)."""
    M = len(mz)
    return 0.5 * (-2 * torch.log(torch.diagonal(Lz)).sum() + (Lz ** 2).sum() + (mz ** 2).sum() - M)


def whitened_KL_batched(mz, Lz):
    """Per-latent whitened KL for mz (..., M), Lz (..., M, M)."""
    M = mz.shape[-1]
    logdiag = torch.log(torch.diagonal(Lz, dim1=-2, dim2=-1)).sum(-1)
    return 0.5 * (-2 * logdiag + (Lz ** 2).sum((-2, -1)) + (mz ** 2).sum(-1) - M)


def svgp_forward(Kxx, Kzz, W, inducing_mean, inducing_cov):
    """mean = W mu (L,N,1); cov = Kxx + sum((W (S - Kzz)) * W, -1) (L,N) for caller-supplied
    matrices (reference utilities.py:382-397).  SVGP.forward does not call this: the fused HIP
    path evaluates the same moments from Linv without forming W or S."""
    mean = W @ inducing_mean.unsqueeze(-1)
    cov = Kxx + ((W @ (inducing_cov - Kzz)) * W).sum(-1)
    return mean, cov


def _kl_u(qU, pU):
    """sum KL(qU || pU); the whitened closed form when the GP returns pU = None (the reference's loops
    call kl_divergence(qU, pU) and therefore only run un-whitened priors)."""
    from torch import distributions
    if pU is None:
        kl = getattr(qU, "_gpz_kl", None)       # the fused pass's own per-latent KL (differentiable), when present
        return kl.sum() if kl is not None else whitened_KL_batched(qU.mean, qU.scale_tril).sum()
    return torch.sum(distributions.kl_divergence(qU, pU))


def _elbo_terms(model, X, y, E, **kwargs):
    """-ELBO of one step exactly as the reference forms it (utilities.py:476-484):
    ``pY.log_prob(y).mean(axis=0).sum()`` -- axis 0 is the sample axis for the Monte-Carlo likelihoods --
    minus KL(qU || pU)."""
    pY, _, qU, pU = model(X=X, E=E, **kwargs)
    return -(pY.log_prob(y).mean(dim=0).sum() - _kl_u(qU, pU))


def _clamp_loadings(model, names=("W", "W2")):
    """keep raw loadings non-negative after an update (utilities.py:522-523, 551-552, 628); a model with real loadings
    (``signed_loadings``: RSF, FA) is left alone"""
    if getattr(model, "signed_loadings", False):
        return
    for n in names:
        w = getattr(model, n, None)
        if isinstance(w, torch.Tensor):
            w.data = torch.clamp(w.data, min=0.0)


def _spots(X, batch_size):
    return torch.multinomial(torch.ones(X.shape[0], device=X.device), num_samples=batch_size, replacement=False)


def _fused_counts_only(model, y, fused):
    """A SparseCounts has no (E,D,N) form: only the fused step takes it.  The same for a SparseExpression."""
    from .likelihoods import SparseCounts, SparseExpression
    if isinstance(y, (SparseCounts, SparseExpression)) and not (fused and hasattr(model, "expected_loglik")):
        raise TypeError(f"{type(y).__name__} goes through the fused step only: pass fused=True to a model with "
                        "expected_loglik (pY.log_prob(y) needs the dense array, y.to_dense())")


class GraphedStep:
    """One optimisation step -- ``loss = loss_fn(); loss.backward(); optimizer.step()`` -- captured ONCE as a HIP graph
    and replayed: at the notebooks' sizes (N ~ 1e3, M ~ 1e2) an eager step is a hundred launches of a few microseconds
    each and the host cannot issue them as fast as the GPU retires them; a replay is one host call.

    What a capture needs, and how it is met: no host synchronisation inside the step (the factorisation's ``info`` word
    and the distributions' argument checks are registered as in ``ops.deferred_info()`` and read after the replay:
    ``check()``); static shapes and the same tensors every step (parameters are updated in place by the optimiser, the
    graph re-reads them); an optimiser whose step counter lives on the device (``capturable=True`` is switched on here
    for torch's Adam-family optimisers -- construct the optimiser, then this object, before any eager step of your own);
    no cross-call factor cache (a captured step factors Kzz at every replay, like the reference).  ``warmup`` eager steps
    run first on the capture stream (they are real steps: ``first_losses`` holds their losses)."""

    def __init__(self, loss_fn, optimizer, warmup: int = 3):
        from . import ops
        params = [p for g in optimizer.param_groups for p in g["params"]]
        dev = params[0].device
        for g in optimizer.param_groups:
            if "capturable" in g:
                g["capturable"] = True
        for st in optimizer.state.values():
            if torch.is_tensor(st.get("step")) and st["step"].device != dev:
                st["step"] = st["step"].to(dev)
        self.optimizer, self.pending = optimizer, ops._DeferredInfo()
        self.first_losses = []
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(max(int(warmup), 1)):        # allocator, library workspaces and optimiser state of this stream
                optimizer.zero_grad(set_to_none=True)
                with ops.deferred_info():
                    loss = loss_fn()
                    loss.backward()
                optimizer.step()
                self.first_losses.append(loss.detach().clone())
            optimizer.zero_grad(set_to_none=True)
            self.graph = torch.cuda.CUDAGraph()
            stack = ops._deferred.__dict__.setdefault("stack", [])
            stack.append(self.pending)
            try:
                with torch.cuda.graph(self.graph, stream=side):
                    loss = loss_fn()
                    loss.backward()
                    optimizer.step()
                    self.loss = loss.detach()
                    bad = self.pending.any_bad()
                    self.bad = bad if bad is not None else torch.zeros((), dtype=torch.bool, device=dev)
                    # what one device-to-host copy per step brings back: the loss and "something needs a look"
                    self.status = torch.stack([self.loss.double(), self.bad.double()])
            finally:
                stack.pop()
        cur.wait_stream(side)

    def __call__(self) -> torch.Tensor:
        """Replay the step; returns the (static) loss tensor of the replayed step -- clone it to keep it."""
        self.graph.replay()
        return self.loss

    def check(self) -> float:
        """One sync: the loss of the last replay as a float; raises what the eager step would have raised
        (torch.linalg.LinAlgError for a Kzz that is not positive-definite, torch's ValueError for invalid distribution
        arguments) -- AFTER that step's parameter update, which is the one difference from the eager loop."""
        loss, bad = self.status.tolist()
        if bad:
            self.pending.check(keep=True)
        return loss


def train(model, optimizer, X, y, device=None, steps=200, E=20, fused=True, sync_losses=True, graph=False, **kwargs):
    """Full-batch optimisation loop with the reference's signature (utilities.py:471-493).  The
    forward and the gradients run on the fused HIP path; the optimiser step is torch's.
    ``fused``: Poisson factor models evaluate ``pY.log_prob(y).mean(0).sum()`` through ``model.expected_loglik``
    (gpz_poisson_nsf: the (E,D,N) rate is never materialised), as the mini-batch loops below do.
    Returns the list of losses: floats, one host sync per step as in the reference (``losses.append(loss.item())``,
    utilities.py:487), or with ``sync_losses=False`` 0-d device tensors converted once at the end -- the same numbers
    without stalling the launch queue every step, which is most of a step at the notebooks' small sizes.
    ``graph``: the step is captured once as a HIP graph and replayed (``GraphedStep``: same objective, same updates;
    the optimiser is switched to ``capturable``; errors surface after the failing step's update instead of before)."""
    from .ops import deferred_info
    _fused_counts_only(model, y, fused)
    losses = []
    if graph and steps > 0:
        def loss_fn():
            if fused and hasattr(model, "expected_loglik"):
                ll, _, qU, pU = model.expected_loglik(X, y, E=E, **kwargs)
                return -(ll - _kl_u(qU, pU))
            return _elbo_terms(model, X, y, E, **kwargs)
        warm = min(3, steps)
        step = GraphedStep(loss_fn, optimizer, warmup=warm)
        dev_losses = list(step.first_losses[:steps])
        bad = None
        for _ in range(steps - warm):
            loss = step()
            if sync_losses:
                dev_losses.append(step.check())
            else:
                dev_losses.append(loss.clone())
                bad = step.bad.clone() if bad is None else bad | step.bad
        if bad is not None and bool(bad):
            step.pending.check(keep=True)
        tens = [v for v in dev_losses if torch.is_tensor(v)]
        vals = iter(torch.stack([t.double() for t in tens]).tolist()) if tens else iter(())
        return [next(vals) if torch.is_tensor(v) else v for v in dev_losses]
    for _ in range(steps):
        optimizer.zero_grad()
        with deferred_info():      # Kzz's `info` is read once, behind the backward pass's launches; a failure raises here
            if fused and hasattr(model, "expected_loglik"):
                ll, _, qU, pU = model.expected_loglik(X, y, E=E, **kwargs)     # (the hybrids' 6-tuples fail here as in the reference)
                loss = -(ll - _kl_u(qU, pU))
            else:
                loss = _elbo_terms(model, X, y, E, **kwargs)
            loss.backward()
        optimizer.step()
        losses.append(loss.item() if sync_losses else loss.detach())
    if not sync_losses and losses:
        losses = torch.stack(losses).tolist()
    return losses


def train_batched(model, optimizer, X, y, device=None, steps=200, E=20, batch_size=1000, fused=True, **kwargs):
    """Mini-batch driver of the Poisson factor models (reference utilities.py:600-632): a fresh subset of
    ``batch_size`` spots per step through ``model.forward_batched``, ``pY.log_prob(y[:, idx]).mean(0).sum()``
    minus KL(qU || pU), ``model.W`` clamped at zero after the update.  ``fused`` evaluates the same
    expected log-likelihood through ``model.expected_loglik`` (gpz_poisson_nsf: the (E,D,N_b) rate is never
    materialised).  The index draw stays on the device (the reference samples on the host every step).
    Models without ``forward_batched`` (plain GP likelihoods) get ``model(X[idx])`` on the sampled spots."""
    from .ops import deferred_info
    _fused_counts_only(model, y, fused)
    losses = []
    for _ in range(steps):
        idx = _spots(X, min(batch_size, X.shape[0]))
        optimizer.zero_grad()
        with deferred_info():
            if not hasattr(model, "forward_batched"):
                kw = dict(kwargs)
                if "groupsX" in kw:
                    kw["groupsX"] = kw["groupsX"][idx]
                loss = _elbo_terms(model, X[idx], y[..., idx], E, **kw)
            else:
                if fused and hasattr(model, "expected_loglik"):
                    ll, _, qU, pU = model.expected_loglik(X, y[:, idx], idx=idx, E=E, **kwargs)
                else:
                    pY, _, qU, pU = model.forward_batched(X=X, idx=idx, E=E, **kwargs)
                    ll = pY.log_prob(y[:, idx]).mean(dim=0).sum()
                loss = -(ll - _kl_u(qU, pU))
            loss.backward()
        optimizer.step()
        _clamp_loadings(model, ("W",))
        losses.append(loss.item())
    return losses


def train_hybrid(model, optimizer, X, y, device=None, steps=200, E=20, fused=True, **kwargs):
    """Full-batch driver of the hybrid (spatial + non-spatial) models, reference utilities.py:530-558."""
    from torch import distributions
    from .ops import deferred_info
    _fused_counts_only(model, y, fused)
    losses = []
    for _ in range(steps):
        optimizer.zero_grad()
        with deferred_info():
            if fused and hasattr(model, "expected_loglik"):
                ll, _, qU, pU, qF, pF = model.expected_loglik(X, y, E=E, **kwargs)
            else:
                pY, _, qU, pU, qF, pF = model(X=X, E=E, **kwargs)
                ll = pY.log_prob(y).mean(dim=0).sum()
            loss = -(ll - _kl_u(qU, pU) - torch.sum(distributions.kl_divergence(qF, pF)))
            loss.backward()
        optimizer.step()
        _clamp_loadings(model)
        losses.append(loss.item())
    return losses


def train_hybrid_batched(model, optimizer, X, y, device=None, steps=200, E=20, batch_size=1000, fused=True, **kwargs):
    """Mini-batch driver of the hybrid models, reference utilities.py:497-527: the log-likelihood is
    ``y log(rate) - rate`` (no log y! term), both KL terms are subtracted, W / W2 are clamped at zero."""
    from torch import distributions
    from .ops import deferred_info
    _fused_counts_only(model, y, fused)
    losses = []
    for _ in range(steps):
        idx = _spots(X, batch_size)
        optimizer.zero_grad()
        with deferred_info():
            if fused and hasattr(model, "expected_loglik"):
                ll, _, qU, pU, qF, pF = model.expected_loglik(X, y[:, idx], idx=idx, E=E, with_lgamma=False, **kwargs)
            else:
                pY, _, qU, pU, qF, pF = model.forward_batched(X=X, idx=idx, E=E, **kwargs)
                ll = (y[:, idx] * torch.log(pY.rate) - pY.rate).mean(dim=0).sum()
            loss = -(ll - _kl_u(qU, pU) - torch.sum(distributions.kl_divergence(qF, pF)))
            loss.backward()
        optimizer.step()
        _clamp_loadings(model)
        losses.append(loss.item())
    return losses


def train_closure_batched(model, optimizer, X, groupsX, y, device=None, steps=200, E=20, batch_size=1000):
    """Closure-style mini-batch driver for optimisers that re-evaluate the loss (LBFGS), multi-group models;
    reference utilities.py:561-597."""
    losses = []

    from .ops import deferred_info

    def closure(idx):
        optimizer.zero_grad()
        with deferred_info():
            pY, _, qU, pU = model.forward_batched(X, groupsX, idx, E=E)
            loss = -(pY.log_prob(y[:, idx]).mean(dim=0).sum() - _kl_u(qU, pU))
            loss.backward()
        losses.append(loss.item())
        return loss

    for _ in range(steps):
        idx = _spots(X, batch_size)
        optimizer.step(lambda: closure(idx))
    return losses


def dims_autocorr(factors, coords, sort=True, *, n_neighs=6, mode="moran"):
    """Moran's I of every column of ``factors`` (N,L) over the directed ``n_neighs``-nearest-neighbour graph of
    ``coords`` (N,d), d <= 4 -- the reference's dims_autocorr (utilities.py:131-156), which builds that graph with
    squidpy's ``spatial_neighbors`` (generic coordinates, 6 neighbours, self excluded) and scores it with
    ``spatial_autocorr(mode="moran")`` (weights 1/n_neighs per row).  Both run here as HIP kernels
    (``ops.spatial_knn``, ``ops.morans_i``) on the GPU of the tensor arguments, or on the current GPU for numpy / host
    inputs.  Neighbours are ranked by (fp64 squared distance, index): sklearn's graph wherever no exact distance tie
    falls on the n_neighs-th place (there its KD-tree's visit order decides).  A constant column gives NaN.

    Returns numpy arrays ``(idx, I)``: idx (L,) int64, I (L,) float64.  ``sort=True``: decreasing I, NaN last, equal
    values in column order (``factors[:, idx]`` orders the factors by spatial autocorrelation).  ``sort=False``: the
    reference's ``df.sort_index()`` over AnnData's default names "0" ... "L-1", which is a STRING sort -- for L >= 11 the
    order is 0, 1, 10, 11, ..., 19, 2, 20, ...; idx and I stay aligned either way.  The reference's
    ``print('here_andata')`` is not reproduced.  For permutation p-values of the factors, score them as genes:
    ``gene_autocorr(factors.T, coords, n_perms=...)``.

    ``mode="geary"`` scores Geary's C instead (``ops.spatial_stats``; squidpy's ``mode="geary"``) and returns ``(idx, C)``;
    ``sort=True`` is then by increasing C -- the most autocorrelated factor first, as with I -- NaN last."""
    import numpy as np
    from . import ops
    if mode not in ("moran", "geary"):
        raise ValueError(f"dims_autocorr: mode={mode!r} unknown ('moran', 'geary')")

    def as_tensor(a):
        return a.detach() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))

    F, X = as_tensor(factors), as_tensor(coords)
    if F.dim() != 2 or X.dim() != 2:
        raise ValueError(f"dims_autocorr: factors (N, L) and coords (N, d) expected, got {tuple(F.shape)} and {tuple(X.shape)}")
    N, L = F.shape
    if X.shape[0] != N:
        raise ValueError(f"dims_autocorr: {N} rows of factors but {X.shape[0]} of coords")
    if not 1 <= X.shape[1] <= 4:
        raise ValueError(f"dims_autocorr: coordinates of dimension {X.shape[1]} unsupported (1..4)")
    k = int(n_neighs)
    if not 1 <= k <= 32:
        raise ValueError(f"dims_autocorr: n_neighs={k} unsupported (1..32)")
    if N <= k:
        raise ValueError(f"dims_autocorr: {N} observations, more than n_neighs={k} needed")
    dev = next((t.device for t in (F, X) if t.is_cuda), None)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if X.dtype not in (torch.float32, torch.float64):
        X = X.double()
    if F.dtype not in (torch.float32, torch.float64):
        F = F.double()
    X, F = X.to(dev), F.to(dev)
    if not bool(torch.isfinite(X).all()):
        raise ValueError("dims_autocorr: coords hold a non-finite value")
    if mode == "geary":
        I = ops.spatial_stats(F, ops.spatial_knn(X, k)).C.cpu().numpy()
    else:
        I = ops.morans_i(F, ops.spatial_knn(X, k)).cpu().numpy()
    if sort:
        order = np.argsort(I if mode == "geary" else -I, kind="stable")      # NaN (-NaN) sorts last; ties keep column order
    else:
        order = np.array(sorted(range(L), key=str), dtype=np.int64)
    return order.astype(np.int64), I[order]


def lnormal_approx_dirichlet(L):
    """(mu, sigma) of the L independent lognormals that match the marginal means and variances of a flat symmetric
    Dirichlet (alpha = L) of dimension L: sigma^2 = log(2 L / (L + 1)), mu = -log(L) - sigma^2 / 2 (both 0 at L = 1);
    reference utilities.py:237-249."""
    import numpy as np
    sigma2 = np.log(2 * L) - np.log(L + 1)
    mu = -np.log(L) - sigma2 / 2.0
    return mu, np.sqrt(sigma2)


def shrink_factors(F, shrinkage=0.2):
    """Rows of F (N,L) pulled towards their own mean, F (1 - a) + a rowsum(F) / L: row sums are kept.  A shrinkage
    outside (0, 1) returns F itself (reference utilities.py:301-306)."""
    a = shrinkage
    if 0 < a < 1:
        F = F * (1 - a) + a * F.sum(axis=1, keepdims=True) / float(F.shape[1])
    return F


def shrink_loadings(W, shrinkage=0.2):
    """Columns of W (D,L) pulled towards their own mean, W (1 - a) + a colsum(W) / D: column sums are kept.  A
    shrinkage outside (0, 1) returns W itself (reference utilities.py:308-313)."""
    a = shrinkage
    if 0 < a < 1:
        W = W * (1 - a) + a * W.sum(axis=0) / float(W.shape[0])
    return W


_NMF_KWARGS = ("solver", "beta_loss", "init", "max_iter", "tol", "random_state", "verbose", "shuffle", "alpha_W", "alpha_H",
               "l1_ratio")


def _nmf_options(kwargs):
    """The sklearn NMF keywords regularized_nmf runs, checked before anything touches a GPU."""
    for k in kwargs:
        if k not in _NMF_KWARGS:
            raise NotImplementedError(f"regularized_nmf: keyword {k!r} is not supported (supported: {', '.join(_NMF_KWARGS)})")
    solver = kwargs.get("solver", "cd")
    if solver != "mu":
        raise NotImplementedError(f"regularized_nmf: solver={solver!r} is not supported: pass solver='mu' (the multiplicative-"
                                  "update solver is the one rebuilt here; sklearn's default 'cd' is not)")
    beta_loss = kwargs.get("beta_loss", "frobenius")
    if not (beta_loss == "kullback-leibler" or (not isinstance(beta_loss, str) and beta_loss == 1)):
        raise NotImplementedError(f"regularized_nmf: beta_loss={beta_loss!r} is not supported: pass "
                                  "beta_loss='kullback-leibler' (or 1); sklearn's default 'frobenius' is not rebuilt")
    if kwargs.get("alpha_W", 0.0) != 0.0:
        raise NotImplementedError(f"regularized_nmf: alpha_W={kwargs['alpha_W']!r} is not supported (only 0.0: no regularisation)")
    alpha_H = kwargs.get("alpha_H", "same")
    if not (alpha_H == "same" or (not isinstance(alpha_H, str) and alpha_H == 0.0)):
        raise NotImplementedError(f"regularized_nmf: alpha_H={alpha_H!r} is not supported (only 'same' or 0.0: no regularisation)")
    init = kwargs.get("init", None)
    if init not in (None, "random", "nndsvd", "nndsvda", "nndsvdar"):
        raise NotImplementedError(f"regularized_nmf: init={init!r} is not supported (None, 'random', 'nndsvd', 'nndsvda', "
                                  "'nndsvdar'; 'custom' starts go through factors= and loadings=)")
    return init, int(kwargs.get("max_iter", 200)), float(kwargs.get("tol", 1e-4)), kwargs.get("random_state", None)


def regularized_nmf(Y, L, sz=1, pseudocount=1e-2, factors=None, loadings=None, shrinkage=0.2, **kwargs):
    """The NSF notebooks' starting values (reference utilities.py:253-299): a KL-divergence NMF of the nonnegative
    (obs x feat) matrix Y with L components, loadings and factors shrunk towards a symmetric Dirichlet, the factors put
    on the log scale (``log(pseudocount + eF) - log(sz)``) and recentred to the lognormal prior mean
    ``lnormal_approx_dirichlet(max(L, 1.1))[0]``, the shift folded into the loadings.  Returns numpy ``(F (N,L), W (D,L))``.

    ``factors`` and ``loadings`` both given: no NMF, only the post-processing, on the host (no GPU needed).  Unlike the
    reference, which scales a float ``loadings`` argument in place when ``shrinkage`` is outside (0, 1), the caller's
    arrays are never modified.

    Y may be ``counts.T`` of a ``likelihoods.SparseCounts`` (the counts the model trains on, held as their non-zeros): the
    start and the updates then run over the stored values in the view's dtype (``counts.T`` float32, ``counts.T.double()``
    float64) through ``ops.counts_matmul`` and ``ops.nmf_kl_mu_sparse`` -- O(nnz L) per iteration, no N x D array -- with
    the same keywords, checks (the values checked are the stored ones), post-processing and output dtypes.  The
    ``SparseCounts`` itself (genes x spots) raises TypeError: there is no silent transposition.

    Otherwise the factorisation runs on the GPU -- Y's own if it is a CUDA tensor, else the current one: float32 stays
    float32, everything else is computed in float64 (as sklearn does); ``nmf.initialize_nmf`` gives sklearn's starting
    values and ``ops.nmf_kl_mu`` (gpz_nmf_kl_update) its multiplicative updates with its stopping rule.  The keywords are
    sklearn's ``NMF``: ``solver='mu'`` and ``beta_loss='kullback-leibler'`` (or 1) are required -- sklearn's defaults,
    coordinate descent on the Frobenius loss, are not rebuilt and raise NotImplementedError rather than return other
    factors; ``init``, ``max_iter`` (200), ``tol`` (1e-4) and ``random_state`` act as in sklearn; ``verbose`` and
    ``shuffle`` are accepted and ignored; ``alpha_W=0.0``, ``alpha_H`` in ('same', 0.0) and ``l1_ratio`` are accepted at
    these no-regularisation values only.  ValueError: Y not 2-D, negative or non-finite entries (checked on the device,
    one synchronisation), L outside 1..64, an NNDSVD init with L > min(N, D).  The output dtypes are the reference's:
    for float32 Y, F is float64 (``np.log(sz)`` is a float64 scalar) and W float32."""
    import numpy as np
    L_int = int(L)
    if factors is None or loadings is None:
        init, max_iter, tol, random_state = _nmf_options(kwargs)
        from . import nmf, ops
        sparse = _transposed_counts(Y, "regularized_nmf")
        Yt = Y if sparse else Y.detach() if isinstance(Y, torch.Tensor) else torch.as_tensor(np.asarray(Y))
        if not sparse and Yt.dim() != 2:
            raise ValueError(f"regularized_nmf: Y must be (obs, feat), got shape {tuple(Yt.shape)}")
        if not 1 <= L_int <= 64:
            raise ValueError(f"regularized_nmf: L={L_int} unsupported (1..64)")
        if init not in (None, "random") and L_int > min(Yt.shape):
            raise ValueError(f"regularized_nmf: init={init!r} needs L <= min(N, D) = {min(Yt.shape)}, got L={L_int}")
        n_sz = np.shape(sz)
        if len(n_sz) and n_sz[0] not in (1, Yt.shape[0]):
            raise ValueError(f"regularized_nmf: {n_sz[0]} size factors for {Yt.shape[0]} observations")
        dev = Yt.device if Yt.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
        if sparse:
            Yt = Yt.to(dev)
            vals = Yt.T.col_val
        else:
            Yt = vals = Yt.to(device=dev, dtype=torch.float32 if Yt.dtype == torch.float32 else torch.float64).contiguous()
        if not bool((torch.isfinite(vals) & (vals >= 0)).all()):
            raise ValueError("regularized_nmf: Y holds a negative or non-finite value")
        W0, H0 = nmf.initialize_nmf(Yt, L_int, init=init, random_state=random_state)
        Wd, Hd, _ = (ops.nmf_kl_mu_sparse if sparse else ops.nmf_kl_mu)(Yt, W0, H0, max_iter=max_iter, tol=tol)
        eF, W = Wd.cpu().numpy(), Hd.cpu().numpy().T
    else:
        eF, W = np.asarray(factors), np.asarray(loadings)
    W = shrink_loadings(W, shrinkage=shrinkage)
    wsum = W.sum(axis=0)
    eF = shrink_factors(eF * wsum, shrinkage=shrinkage)
    F = np.log(pseudocount + eF) - np.log(sz)
    shift = F.mean(axis=0) - lnormal_approx_dirichlet(max(L, 1.1))[0] * np.ones(L_int)
    F = F - shift
    scale = np.exp(shift - np.log(wsum))
    W = (W * scale).astype(W.dtype, copy=False) if np.issubdtype(W.dtype, np.floating) else W * scale
    return F, W


def init_softplus(mat, minval=1e-5):
    """A copy of the numpy array ``mat`` with every entry x < 20 replaced by ``log(exp(x) - 1 + minval)``, the inverse
    of softplus floored by ``minval``: raw parameters whose softplus is ``mat`` (reference utilities.py:38-43).  Entries
    >= 20 are their own inverse to rounding and stay."""
    import numpy as np
    out = np.array(mat, copy=True)
    small = out < 20
    out[small] = np.log(np.exp(out[small]) - 1 + minval)
    return out


def _transposed_counts(Y, who):
    """True for ``counts.T`` of a ``SparseCounts``; the ``SparseCounts`` itself (genes x spots) is refused, not transposed."""
    from .likelihoods import SparseCounts, TransposedCounts, _counts_expected
    _counts_expected(Y, who)
    if isinstance(Y, SparseCounts):
        raise TypeError(f"{who}: Y is a SparseCounts (genes x spots); pass its .T (obs x feat)")
    return isinstance(Y, TransposedCounts)


def _spot_totals_tensor(c):
    """(N,) fp64 totals of the spots of a whole ``SparseCounts``, on its device: segment sums of the stored values."""
    run = torch.cat([c.col_val.new_zeros(1, dtype=torch.float64), torch.cumsum(c.col_val.to(torch.float64), 0)])
    return torch.diff(run[c.col_ptr])


def _spot_totals(Y, who="train_val_split"):
    """(N,1) row totals of Y (obs x feat): numpy's own sum, or of ``counts.T`` the fp64 segment sums of the stored values."""
    if _transposed_counts(Y, who):
        return _spot_totals_tensor(Y.T).cpu().numpy().reshape(-1, 1)
    return Y.sum(axis=1, keepdims=True)


def scanpy_sizefactors(Y):
    """(N,1) size factors of the count matrix Y (obs x feat): the row totals over their median (reference
    utilities.py:232-234).  Y may be ``counts.T`` of a ``SparseCounts``: the spot totals are then the fp64 segment sums of
    the stored values on the counts' device, and the (N,1) float64 numpy array comes back."""
    import numpy as np
    totals = _spot_totals(Y, "scanpy_sizefactors")
    return totals / np.median(totals)


def log_normalize(counts, size_factors=None, center=True, offset=None):
    """The normalisation the nsf paper feeds to RSF / MEFISTO / FA -- log1p of size-normalised counts, centred per gene --
    of a whole ``SparseCounts``, as a ``SparseExpression``: ``z = log1p(y / sz[n])`` on the stored entries only (a zero
    count stays zero, so z has exactly the sparsity of the counts) and the centring as the (D,) fp64 ``offset``.  O(nnz):
    the index arrays are shared with ``counts``, only the values are new (formed in fp64, stored in fp32).

    ``size_factors``: (N,) positive; default ``scanpy_sizefactors(counts.T)`` (a spot without counts has no stored entry,
    so nothing divides by zero).  ``center=True``: ``offset`` = the per-gene mean of z over all N spots (fp64 segment sums);
    ``center=False``: zeros.  ``offset=``: a given (D,) tensor instead, e.g. the training split's means for a held-out
    split.  Views, dense tensors and a ``SparseExpression`` raise TypeError."""
    from .likelihoods import SparseCounts, SparseExpression, _gene_moments
    if not isinstance(counts, SparseCounts) or counts.base is not counts:
        what = "a view y[:, idx]" if isinstance(counts, SparseCounts) else type(counts).__name__
        raise TypeError(f"log_normalize: a whole SparseCounts expected, got {what} (build one with SparseCounts(y))")
    D, N = counts.shape
    dev = counts.device
    if size_factors is None:
        size_factors = scanpy_sizefactors(counts.T)
    sz = torch.as_tensor(size_factors).detach().reshape(-1).to(device=dev, dtype=torch.float64)
    if sz.numel() != N:
        raise ValueError(f"log_normalize: {sz.numel()} size factors for {N} spots")
    values = object.__new__(SparseCounts)
    values.base, values.idx, values.pos, values.shape = values, None, None, counts.shape
    for k in SparseCounts._PARTS:
        setattr(values, k, getattr(counts, k))
    values.col_val = torch.log1p(counts.col_val.to(torch.float64) / sz[counts._spots()]).to(torch.float32)
    if offset is not None:
        off = torch.as_tensor(offset).detach().reshape(-1).to(device=dev, dtype=torch.float64)
        if off.numel() != D:
            raise ValueError(f"log_normalize: offset has {off.numel()} values for {D} genes")
    elif center:
        off = _gene_moments(SparseExpression(values, torch.zeros(D, dtype=torch.float64, device=dev)))[0] / N
    else:
        off = torch.zeros(D, dtype=torch.float64, device=dev)
    return SparseExpression(values, off)


def _whole_counts_only(counts, who):
    """A whole ``SparseCounts``, or TypeError: a ``SparseExpression`` holds no counts (``_counts_expected``), ``counts.T``
    and views are not the (genes, spots) data set."""
    from .likelihoods import SparseCounts, TransposedCounts, _counts_expected
    _counts_expected(counts, who)
    if isinstance(counts, TransposedCounts):
        raise TypeError(f"{who}: counts is the .T (obs x feat) of a SparseCounts; pass the SparseCounts itself (genes x spots)")
    if not isinstance(counts, SparseCounts):
        raise TypeError(f"{who}: a whole SparseCounts expected, got {type(counts).__name__} (build one with SparseCounts(y))")
    if counts.base is not counts:
        raise TypeError(f"{who}: counts is a view y[:, idx]; the whole SparseCounts is needed")
    return counts


def _gene_sizes(c, size_factors, who):
    """The (N,) fp64 sizes of the spots on the counts' device: None = the spots' total counts, else an (N,) or (N, 1) array
    of positive finite values."""
    N = c.shape[1]
    if size_factors is None:
        return _spot_totals_tensor(c)
    import numpy as np
    sf = size_factors.detach() if isinstance(size_factors, torch.Tensor) else torch.as_tensor(np.asarray(size_factors))
    if tuple(sf.shape) not in ((N,), (N, 1)):
        raise ValueError(f"{who}: size_factors of shape {tuple(sf.shape)} for {N} spots ((N,) or (N, 1) expected)")
    size = sf.reshape(-1).to(device=c.device, dtype=torch.float64)
    if not bool((size > 0).all() & torch.isfinite(size).all()):
        raise ValueError(f"{who}: size_factors must be positive and finite")
    return size


_DEVIANCE_FAMILIES = {"poisson": 0, "binomial": 1}


def gene_deviance(counts, family="poisson", size_factors=None):
    """(D,) fp64 deviance of every gene of a whole ``SparseCounts`` against a constant-rate null, on the counts' device
    (``ops.gene_deviance_sparse``) -- scry's ``devianceFeatureSelection``, the ranking the nsf paper selects genes with and
    the reference's ``anndata_to_train_val`` expects to have happened ("features sorted in decreasing importance").  Sums
    over the stored counts only; a gene without counts scores 0.

    ``family``: "poisson", or "binomial" (scry's default; the size of a spot is then its total count).  ``size_factors``:
    None = the spots' total counts (required for "binomial"), else an (N,) or (N, 1) array of positive values.  A
    ``SparseExpression``, ``counts.T`` or a view raises TypeError."""
    from . import ops
    c = _whole_counts_only(counts, "gene_deviance")
    if family not in _DEVIANCE_FAMILIES:
        raise ValueError(f"gene_deviance: family {family!r} unknown ('poisson', 'binomial')")
    if size_factors is not None and family == "binomial":
        raise ValueError("gene_deviance: the binomial deviance takes the spots' total counts as sizes (size_factors=None)")
    size = _gene_sizes(c, size_factors, "gene_deviance")
    return ops.gene_deviance_sparse(c, size.contiguous(), _DEVIANCE_FAMILIES[family])[2]


class GeneDispersion(NamedTuple):
    """``gene_dispersion``: the negative-binomial fit of every gene under the constant-rate null, (D,) tensors on the counts'
    device.  ``theta`` fp64: the maximum-likelihood inverse dispersion, +inf where the gene shows no overdispersion below the
    range's upper end, NaN for a gene without counts; ``loglik`` = ``poisson_loglik`` + gain at that theta; ``lr`` = 2 gain,
    the likelihood-ratio statistic against Poisson; ``pvalue`` = erfc(sqrt(gain)) / 2, its tail under the boundary mixture
    (chi2_0 + chi2_1) / 2 (1 at the Poisson limit); ``status`` int32 (0 interior root, 1 Poisson limit, 2 at the range's
    lower end, 3 not converged, 4 no counts) and ``iterations`` int32 (score evaluations after the two at the ends)."""
    theta: torch.Tensor
    loglik: torch.Tensor
    poisson_loglik: torch.Tensor
    lr: torch.Tensor
    pvalue: torch.Tensor
    status: torch.Tensor
    iterations: torch.Tensor


def gene_dispersion(counts, size_factors=None, *, theta_range=(1e-4, 1e6), max_iter=50):
    """The gene-wise negative-binomial inverse dispersion of a whole ``SparseCounts`` by maximum likelihood, on the counts'
    device (``ops.gene_dispersion_sparse``) -- what edgeR, DESeq2 and glmGamPoi's ``overdispersion_mle`` compute on the host,
    with the rate of gene d held at the null of ``gene_deviance``: mu_dn = p_d size_n, p_d = sum_n y_dn / sum_n size_n.  It
    answers which genes are overdispersed at all (``pvalue``, ``lr``: is ``likelihood="nb"`` worth its cost over Poisson?)
    and where theta can start for each gene (``theta0=`` of the count models).  The null absorbs all biological variation
    of a gene into its dispersion, so ``theta`` is a lower-biased start for a factor model's theta, not an estimate of it.

    ``size_factors``: None = the spots' total counts, else an (N,) or (N, 1) array of positive values.  ``theta_range``:
    the interval theta is sought in.  ``max_iter`` <= 200: score evaluations per gene.  Returns a ``GeneDispersion``.  A
    ``SparseExpression``, ``counts.T`` or a view raises TypeError."""
    import math
    from . import ops
    c = _whole_counts_only(counts, "gene_dispersion")
    try:
        lo, hi = (float(v) for v in theta_range)
    except (TypeError, ValueError):
        raise ValueError(f"gene_dispersion: theta_range {theta_range!r} must be (theta_min, theta_max)") from None
    if not (0.0 < lo < hi and math.isfinite(hi)):
        raise ValueError(f"gene_dispersion: theta_range ({lo}, {hi}) unsupported (0 < theta_min < theta_max, both finite)")
    size = _gene_sizes(c, size_factors, "gene_dispersion")
    theta, gain, pl, status, iterations = ops.gene_dispersion_sparse(c, size.contiguous(), lo, hi, max_iter)
    pvalue = 0.5 * torch.erfc(torch.sqrt(gain.clamp_min(0.0)))
    pvalue = torch.where(status == 1, torch.ones_like(pvalue), pvalue)            # theta = inf: the chi2_0 half, all of it
    pvalue = torch.where(status == 4, torch.full_like(pvalue, float("nan")), pvalue)
    return GeneDispersion(theta, pl + gain, pl, 2.0 * gain, pvalue, status, iterations)


class GeneSpatialGP(NamedTuple):
    """``gene_spatial_gp``: the sparse-GP fit of every gene, tensors on the values' device.  (D,) at each gene's best length
    scale: ``lengthscale`` fp64 and ``ell_index`` int64 into ``lengthscales``; ``loglik`` the collapsed bound there,
    ``null_loglik`` the model without a spatial term, ``lr`` = 2 (loglik - null_loglik) >= 0, ``pvalue`` = erfc(sqrt(lr / 2));
    ``s2`` and ``tau2`` the spatial and the noise variance, ``delta`` = tau2 / s2, ``fsv`` the fraction of spatial variance
    s2 gamma / (s2 gamma + tau2); ``status`` int32 (0 interior, 1 no spatial variance in the delta range, 2 at its lower
    end, 3 degenerate: a constant gene, NaN in every value).  ``loglik_grid`` (D, n_ell) the bound at every length scale,
    ``lengthscales`` (n_ell,), ``Z`` (M, d)."""
    lengthscale: torch.Tensor
    ell_index: torch.Tensor
    loglik: torch.Tensor
    null_loglik: torch.Tensor
    lr: torch.Tensor
    pvalue: torch.Tensor
    s2: torch.Tensor
    tau2: torch.Tensor
    delta: torch.Tensor
    fsv: torch.Tensor
    status: torch.Tensor
    loglik_grid: torch.Tensor
    lengthscales: torch.Tensor
    Z: torch.Tensor


def _default_lengthscales(X, M, n=8):
    """n geometric steps from the inducing-point spacing h = (bounding-box volume / M)^(1/d) to half the longest side."""
    import math
    side = (X.max(dim=0).values - X.min(dim=0).values).clamp_min(torch.finfo(torch.float64).tiny)
    d = X.shape[1]
    h = float(torch.exp(torch.log(side).sum() / d)) / float(M) ** (1.0 / d)
    top = 0.5 * float(side.max())
    if not h < top:
        return torch.tensor([top], dtype=torch.float64, device=X.device)
    return torch.exp(torch.linspace(math.log(h), math.log(top), n, dtype=torch.float64, device=X.device))


def _eigh(B):
    """``torch.linalg.eigh`` where B lives, on the host if the device build lacks it."""
    try:
        return torch.linalg.eigh(B)
    except RuntimeError:
        lam, U = torch.linalg.eigh(B.cpu())
        return lam.to(B.device), U.to(B.device)


def gene_spatial_gp(values, coords, *, inducing=256, kernel="rbf", lengthscales=None, delta_range=(1e-3, 1e6), jitter=1e-6,
                    seed=0):
    """Is a gene spatially variable under a Gaussian process, at what length scale, and with what fraction of its variance
    -- SpatialDE's and nnSVG's question, for every gene at once on the values' device and at sparse-GP cost.  One gene is
    y (N,), centred expression; the model is y = f + eps, f ~ GP(0, s2 k_l), eps ~ N(0, tau2 I) with a unit-variance
    stationary ``kernel`` ("rbf", "matern12", "matern32", "matern52") and inducing points Z, scored by Titsias' collapsed
    variational bound -- the ELBO of this library's ``SVGP`` with a Gaussian likelihood at the optimal q(u), a lower bound of
    the exact marginal likelihood.  s2 is profiled out in closed form, delta = tau2 / s2 is maximised per (gene, length
    scale) over ``delta_range`` (``ops.gene_gp_profile``), the length scale over the grid ``lengthscales``.  The answers are
    also a model's set-up: ``lengthscale=`` of its kernel, which genes belong in the spatial half of a hybrid, how many
    inducing points resolve the structure that is there.

    ``values``: a whole ``SparseExpression`` (``log_normalize(counts)``), or a dense (D, N) tensor, whose non-zeros are stored
    and which is centred per gene.  A ``SparseCounts`` raises TypeError (normalise it with ``log_normalize``), as do views
    and ``.T``.  ``coords`` (N, d), d <= 4.  ``inducing``: an (M, d) tensor used as Z, or an int M for
    ``kmeans_inducing_points(coords, M, random_state=seed)``; M <= 1024.  ``lengthscales``: up to 16 values; default 8
    geometric steps from the inducing-point spacing h = (bounding-box volume / M)^(1/d) to half the longest side of the
    bounding box.  A sparse GP cannot see structure finer than h: a gene that varies below it looks like noise here, and a
    length scale under h only weakens the bound -- take more inducing points to look finer.

    The N-dependent work is two passes: K_zx K_xz and K_zx 1 from ``ops.kernel_gram`` (fp64,
    one "latent" per length scale) and K_zx Y^T over the stored entries from ``ops.gene_kernel_project_sparse`` (above 290 N
    stored entries, where the plan finds it faster, from a K_xz filled per length scale and gathered by
    ``ops.counts_matmul``: N x M x 8 bytes at a time); the rest is
    M x M algebra in fp64 (``ops.cholesky``, triangular solves, ``torch.linalg.eigh`` of the n_ell matrices Phi Phi^T --
    on the host if the device build lacks it -- and one matmul for the rotation).  A gene then costs M terms per
    evaluation of the bound, whatever N is.

    Returns a ``GeneSpatialGP``.  ``pvalue`` = erfc(sqrt(lr / 2)) is the chi2_1 tail SpatialDE uses.  It ignores that lr is
    a maximum over the length-scale grid, that s2 >= 0 is a boundary of the parameter space, and that a bound stands in place
    of the likelihood: it ranks and screens genes (put ``fdr_bh`` on top of it), it is not a calibrated test.  ``fsv`` uses
    the Gower factor gamma = (sum lam - |Phi 1|^2 / N) / (N - 1) of Phi^T Phi.  y.y is formed as sum z^2 - 2 offset sum z +
    N offset^2: for a nearly constant gene it loses digits in proportion to mean^2 / variance, as Moran's I does here."""
    import math
    from . import ops
    from .likelihoods import SparseCounts, SparseExpression, TransposedCounts, _gene_moments
    who = "gene_spatial_gp"
    if isinstance(values, TransposedCounts):
        raise TypeError(f"{who}: values is a .T (obs x feat); pass the (genes x spots) SparseExpression itself")
    if isinstance(values, SparseCounts):
        raise TypeError(f"{who}: a SparseCounts holds counts; pass log_normalize(counts), a SparseExpression")
    if isinstance(values, SparseExpression):
        if values.is_view:
            raise TypeError(f"{who}: values is a view y[:, idx]; the whole SparseExpression is needed")
        expr = values
    elif isinstance(values, torch.Tensor):
        if values.dim() != 2 or not values.is_floating_point():
            raise TypeError(f"{who}: a dense (D, N) floating-point tensor expected, got {values.dtype} of shape {tuple(values.shape)}")
        stored = SparseCounts(values.detach())                     # fp32 values; the means are those of what is stored
        zero = torch.zeros(stored.shape[0], dtype=torch.float64, device=stored.device)
        expr = SparseExpression(stored, _gene_moments(SparseExpression(stored, zero))[0] / stored.shape[1])
    else:
        raise TypeError(f"{who}: a whole SparseExpression or a dense (D, N) tensor expected, got {type(values).__name__}")
    kind = ops._gene_gp_kind(who, kernel)
    D, N = expr.shape
    X = torch.as_tensor(coords).detach()
    if X.dim() != 2 or X.shape[0] != N or not 1 <= X.shape[1] <= 4:
        raise ValueError(f"{who}: coords ({N}, d) with 1 <= d <= 4 expected, got {tuple(X.shape)}")
    if N < 2:
        raise ValueError(f"{who}: {N} spot; at least 2 are needed")
    try:
        d_lo, d_hi = (float(v) for v in delta_range)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: delta_range {delta_range!r} must be (delta_min, delta_max)") from None
    if not (0.0 < d_lo < d_hi and math.isfinite(d_hi)):
        raise ValueError(f"{who}: delta_range ({d_lo}, {d_hi}) unsupported (0 < delta_min < delta_max, both finite)")
    if not float(jitter) >= 0.0:
        raise ValueError(f"{who}: jitter={jitter!r} must be >= 0")
    dev = expr.device
    X = X.to(device=dev, dtype=torch.float64).contiguous()
    if isinstance(inducing, torch.Tensor):
        Z = inducing.detach().to(device=dev, dtype=torch.float64).contiguous()
        if Z.dim() != 2 or Z.shape[1] != X.shape[1]:
            raise ValueError(f"{who}: inducing (M, {X.shape[1]}) expected, got {tuple(Z.shape)}")
    elif isinstance(inducing, int) and not isinstance(inducing, bool):
        if not 1 <= inducing <= min(N, 1024):
            raise ValueError(f"{who}: inducing={inducing} outside [1, min(N, 1024)]")
        Z = kmeans_inducing_points(X, inducing, random_state=seed).contiguous()
    else:
        raise TypeError(f"{who}: inducing must be an int or an (M, d) tensor, got {type(inducing).__name__}")
    M = int(Z.shape[0])
    if not 1 <= M <= 1024:
        raise ValueError(f"{who}: M={M} inducing points unsupported (1..1024)")
    if lengthscales is None:
        ell = _default_lengthscales(X, M)
    else:
        ell = torch.as_tensor(lengthscales).detach().reshape(-1).to(device=dev, dtype=torch.float64).contiguous()
        if not 1 <= ell.numel() <= 16 or not bool((ell > 0).all() & torch.isfinite(ell).all()):
            raise ValueError(f"{who}: lengthscales must be 1..16 positive finite values")
    nl = int(ell.numel())

    spec = ops.KernelSpec(kind, torch.ones(nl, dtype=torch.float64, device=dev), ell, True)
    G, b = ops.kernel_gram(spec, Z, X, torch.ones((nl, N), dtype=torch.float64, device=dev), 0.0)     # K_zx K_xz, K_zx 1
    Kzz = ops.kfill(spec, Z, Z) + float(jitter) * torch.eye(M, dtype=torch.float64, device=dev)
    Lz = torch.tril(ops.cholesky(Kzz))
    B = ops.solve_triangular_lower(Lz, ops.solve_triangular_lower(Lz, G).transpose(-1, -2).contiguous())   # Lz^-1 G Lz^-T
    lam, U = _eigh(0.5 * (B + B.transpose(-1, -2)))
    lam = lam.clamp_min(0.0).contiguous()
    W = torch.linalg.solve_triangular(Lz.transpose(-1, -2), U, upper=True)                            # Lz^-T U
    phi1 = ops.solve_triangular_lower(Lz, b.transpose(-1, -2).contiguous())[:, :, 0]                   # Phi 1, (n_ell, M)

    generate = ops.gene_kernel_project_plan(N, D, expr.nnz, M, nl)["generate"]          # the plan's rule: which way is faster
    P = (ops.gene_kernel_project_sparse if generate else ops.gene_kernel_project_gather)(expr, X, Z, ell, kernel)   # K_zx z^T
    P -= expr.offset[None, :, None] * b                                                               # K_zx y^T
    p = torch.matmul(P, W)                                                                            # U^T Phi y
    del P
    sz, szz = _gene_moments(expr)
    yty = (szz - 2.0 * expr.offset * sz + N * expr.offset * expr.offset).contiguous()
    F, delta, s2, tau2, status, _ = ops.gene_gp_profile(p, lam, yty, N, d_lo, d_hi)

    best = torch.where(torch.isnan(F), torch.full_like(F, -float("inf")), F).argmax(dim=1)
    pick = lambda t: t.gather(1, best[:, None])[:, 0]
    loglik = pick(F)
    null = -0.5 * N * (torch.log(2.0 * math.pi * yty / N) + 1.0)
    null = torch.where(yty > 0, null, torch.full_like(null, float("nan")))
    lr = (2.0 * (loglik - null)).clamp_min(0.0)
    gamma = ((lam.sum(dim=1) - (phi1 * phi1).sum(dim=1) / N) / (N - 1))[best]
    s2b, tau2b = pick(s2), pick(tau2)
    return GeneSpatialGP(ell[best], best, loglik, null, lr, torch.erfc(torch.sqrt(0.5 * lr)), s2b, tau2b, pick(delta),
                         s2b * gamma / (s2b * gamma + tau2b), pick(status), F, ell, Z)


class GeneAutocorr(NamedTuple):
    """``gene_autocorr``: Moran's I per gene and the moments squidpy reports beside it under the normality assumption
    (they depend on the graph alone), all fp64 tensors: ``I`` (D,), ``expected`` = -1 / (N - 1), ``variance`` (scalars) and
    ``z`` = (I - expected) / sqrt(variance) (D,)."""
    I: torch.Tensor
    expected: torch.Tensor
    variance: torch.Tensor
    z: torch.Tensor


def _moran_moments(nbr):
    """(expected, variance) of Moran's I under normality for row-normalised weights 1 / K over the table nbr (N, K) of
    distinct neighbours without self edges, from integer counts: S0 = N, S1 = (N K + 2 m) / K^2 with m mutual pairs,
    S2 = sum_i (1 + indeg_i / K)^2; fp64 scalars on the table's device."""
    N, K = nbr.shape
    rows = torch.arange(N, dtype=torch.int64, device=nbr.device)[:, None]
    forward, backward = (rows * N + nbr).reshape(-1), (nbr * N + rows).reshape(-1)
    m2 = int(torch.isin(forward, backward).sum())                 # directed edges whose reverse is an edge too: 2 m
    indeg = torch.bincount(nbr.reshape(-1), minlength=N).to(torch.float64)
    S0 = float(N)
    S1 = (N * K + m2) / float(K * K)
    S2 = ((1.0 + indeg / K) ** 2).sum()
    expected = torch.tensor(-1.0 / (N - 1), dtype=torch.float64, device=nbr.device)
    variance = (N * N * S1 - N * S2 + 3.0 * S0 * S0) / ((N * N - 1.0) * S0 * S0) - expected * expected
    return expected, variance


class GeneAutocorrPerm(NamedTuple):
    """``gene_autocorr(..., n_perms=)``: the fields of ``GeneAutocorr`` (``I``, ``expected``, ``variance``, ``z``: what the
    call without permutations returns, bit for bit) and the permutation null of squidpy's ``spatial_autocorr(n_perms=)``,
    (D,) tensors on the values' device.  ``n_perms`` = P (int); ``n_ge`` / ``n_le`` int32: the permutations whose I is >= /
    <= the observed one; ``pval_greater`` = (n_ge + 1) / (P + 1), ``pval_less`` = (n_le + 1) / (P + 1), ``pval_sim`` the
    smaller of the two (squidpy's folded pseudo p-value, identical to it when no simulation ties with I); ``mean_sim`` and
    ``var_sim`` (the population variance, as ``np.var``) of the simulated I; ``z_sim`` = (I - mean_sim) / sqrt(var_sim), NaN
    where var_sim is 0; ``pval_z_sim`` = erfc(|z_sim| / sqrt 2) / 2; ``sims`` (D, P) fp64 or None.  A gene whose I is NaN has
    NaN p-values and zero counts."""
    I: torch.Tensor
    expected: torch.Tensor
    variance: torch.Tensor
    z: torch.Tensor
    n_perms: int
    n_ge: torch.Tensor
    n_le: torch.Tensor
    pval_greater: torch.Tensor
    pval_less: torch.Tensor
    pval_sim: torch.Tensor
    mean_sim: torch.Tensor
    var_sim: torch.Tensor
    z_sim: torch.Tensor
    pval_z_sim: torch.Tensor
    sims: Optional[torch.Tensor]


class GeneGeary(NamedTuple):
    """``gene_autocorr(mode="geary")``: Geary's C per gene and its moments, fp64 tensors: ``C`` (D,), ``expected`` = 1,
    ``variance`` (a scalar under normality, (D,) under randomisation) and ``z`` = (C - 1) / sqrt(variance) (D,).  Mind the
    sign: C < 1, a NEGATIVE z, is positive spatial autocorrelation (neighbours are alike); C > 1 is negative."""
    C: torch.Tensor
    expected: torch.Tensor
    variance: torch.Tensor
    z: torch.Tensor


class GeneGearyPerm(NamedTuple):
    """``gene_autocorr(mode="geary", n_perms=)``: the fields of ``GeneAutocorrPerm`` with ``C`` for ``I``.  ``n_ge`` /
    ``n_le`` count the permutations whose C is >= / <= the observed one, so ``pval_less`` = (n_le + 1) / (P + 1) is the one
    for positive autocorrelation (a small C), ``pval_greater`` the one for negative; ``pval_sim`` is the smaller of the two."""
    C: torch.Tensor
    expected: torch.Tensor
    variance: torch.Tensor
    z: torch.Tensor
    n_perms: int
    n_ge: torch.Tensor
    n_le: torch.Tensor
    pval_greater: torch.Tensor
    pval_less: torch.Tensor
    pval_sim: torch.Tensor
    mean_sim: torch.Tensor
    var_sim: torch.Tensor
    z_sim: torch.Tensor
    pval_z_sim: torch.Tensor
    sims: Optional[torch.Tensor]


def _autocorr_moments(nbr, kurtosis=None):
    """The moments of Moran's I and Geary's C over the table nbr (N, K) of distinct neighbours without self edges, the
    sibling of ``_moran_moments``: a dict of fp64 tensors on the table's device with ``EI`` = -1 / (N - 1), ``EC`` = 1, the
    normality variances ``VI_norm`` and ``VC_norm`` (scalars) and, with ``kurtosis`` (the (D,) b2 of the genes; N >= 4), the
    randomisation variances ``VI_rand`` and ``VC_rand`` (D,) -- the exact variances over all N! relabellings of the spots
    (Cliff & Ord; PySAL's VI_rand, VC_rand).  Binary weights (both ratios are the same for weights 1 / K):
    S0 = N K, S1 = N K + m2 with m2 directed edges whose reverse is an edge, S2 = sum_i (K + indeg_i)^2, counted once as
    integers; every variance is a - b2 b with a and b exact rationals of those, rounded once."""
    from fractions import Fraction as Fr
    n, K = (int(v) for v in nbr.shape)
    rows = torch.arange(n, dtype=torch.int64, device=nbr.device)[:, None]
    forward, backward = (rows * n + nbr).reshape(-1), (nbr * n + rows).reshape(-1)
    indeg = torch.bincount(nbr.reshape(-1), minlength=n)
    S0, S1, S2 = n * K, n * K + int(torch.isin(forward, backward).sum()), int(((K + indeg) ** 2).sum())

    def t(v):
        return torch.tensor(float(v), dtype=torch.float64, device=nbr.device)

    EI2 = Fr(1, (n - 1) ** 2)
    out = dict(EI=t(Fr(-1, n - 1)), EC=t(1), S0=S0, S1=S1, S2=S2,
               VI_norm=t(Fr(n * n * S1 - n * S2 + 3 * S0 * S0, (n * n - 1) * S0 * S0) - EI2),
               VC_norm=t(Fr((2 * S1 + S2) * (n - 1) - 4 * S0 * S0, 2 * (n + 1) * S0 * S0)))
    if kurtosis is not None:
        if n < 4:
            raise ValueError(f"the randomisation variance needs N >= 4 spots, got {n}")
        b2 = kurtosis.to(torch.float64)
        dI, dC = (n - 1) * (n - 2) * (n - 3) * S0 * S0, n * (n - 2) * (n - 3) * S0 * S0
        aI = Fr(n * ((n * n - 3 * n + 3) * S1 - n * S2 + 3 * S0 * S0), dI) - EI2
        bI = Fr((n * n - n) * S1 - 2 * n * S2 + 6 * S0 * S0, dI)
        aC = Fr(4 * (n - 1) * S1 * (n * n - 3 * n + 3) - (n - 1) * S2 * (n * n + 3 * n - 6) + 4 * S0 * S0 * (n * n - 3), 4 * dC)
        bC = Fr(4 * (n - 1) ** 2 * S1 - (n - 1) * S2 * (n * n - n + 2) + 4 * S0 * S0 * (n - 1) ** 2, 4 * dC)
        out["VI_rand"] = t(aI) - b2 * t(bI)
        out["VC_rand"] = t(aC) - b2 * t(bC)
    return out


def _ring(N, device):
    """The (N, 1) table i -> i + 1 mod N: a valid graph for a call that wants the moments of the values alone."""
    return ((torch.arange(N, dtype=torch.int64, device=device) + 1) % N)[:, None].contiguous()


def gene_kurtosis(values):
    """(D,) fp64 kurtosis b2 = m4 / m2^2 of every gene, zeros included (m_k = sum (x - mean)^k / N; 3 for a normal sample):
    what the randomisation variance of ``gene_autocorr(assumption="randomisation")`` depends on beside the graph.
    ``values`` as for ``gene_autocorr``: a whole ``SparseCounts`` / ``SparseExpression``, swept twice over its stored entries
    (``ops.gene_spatial_stats_sparse``), or a dense (D, N) tensor (``ops.spatial_stats``).  NaN for a constant gene."""
    from . import ops
    from .likelihoods import SparseCounts, SparseExpression
    if isinstance(values, (SparseCounts, SparseExpression)):
        v = ops._whole_values(values, "gene_kurtosis")
        if v.shape[1] < 2:
            raise ValueError("gene_kurtosis: at least 2 spots needed")
        return ops.gene_spatial_stats_sparse(values, _ring(v.shape[1], v.device)).kurtosis
    if not isinstance(values, torch.Tensor) or values.dim() != 2 or not values.is_floating_point() or values.shape[1] < 2:
        raise ValueError("gene_kurtosis: a SparseCounts, a SparseExpression or a dense (D, N >= 2) floating-point tensor expected")
    V = values.detach()
    V = (V if V.dtype in (torch.float32, torch.float64) else V.float()).T.contiguous()
    return ops.spatial_stats(V, _ring(V.shape[0], V.device)).kurtosis


def _autocorr_perms(who, N, n_perms, perms):
    """The checked arguments of the permutation null: (P, perms or None)."""
    import numpy as np
    if n_perms is not None and perms is not None:
        raise ValueError(f"{who}: n_perms and perms exclude each other (perms carries its own count)")
    if perms is not None:
        pm = perms.detach() if isinstance(perms, torch.Tensor) else torch.as_tensor(np.asarray(perms))
        if pm.dim() != 2 or pm.shape[0] < 1 or pm.shape[1] != N or pm.dtype.is_floating_point or pm.dtype == torch.bool:
            raise ValueError(f"{who}: perms must be a (P, {N}) integer tensor, P >= 1, got {tuple(pm.shape)} of {pm.dtype}")
        return int(pm.shape[0]), pm
    if isinstance(n_perms, bool) or not isinstance(n_perms, int) or n_perms < 1:
        raise ValueError(f"{who}: n_perms={n_perms!r} must be a positive integer")
    return n_perms, None


def gene_autocorr(values, coords=None, *, n_neighs=6, graph=None, n_perms=None, seed=0, perms=None, return_sims=False,
                  mode="moran", assumption="normality"):
    """Moran's I of every gene over the spots' directed ``n_neighs``-nearest-neighbour graph -- squidpy's
    ``spatial_autocorr(mode="moran")`` with one gene per column, the other standard ranking of spatial data.  ``values``: a
    whole ``SparseCounts`` or ``SparseExpression`` (the offset does not change I), scored from its stored entries
    (``ops.gene_morans_i_sparse``; nothing of D x N elements is formed), or a dense (D, N) tensor, scored by
    ``ops.morans_i``.  The graph is ``ops.spatial_knn(coords, n_neighs)`` (``coords`` (N, d), d <= 4), or ``graph=``, an
    (N, K) int64 table of distinct neighbours, K <= 32.  Returns a ``GeneAutocorr``.  A gene without stored entries and a
    constant gene give NaN; I of a nearly constant gene loses digits in proportion to mean^2 / variance.

    ``n_perms=P`` (or ``perms=``, a (P, N) integer tensor of permutations, used as given) adds the permutation null of
    squidpy's ``spatial_autocorr(..., n_perms=)`` and returns a ``GeneAutocorrPerm``: I is recomputed under P random
    relabellings of the spots (``ops.gene_morans_perm_sparse`` over the stored entries, ``ops.morans_perm_rows`` for a dense
    tensor, which is scored in fp32), in O(entries x K) per permutation.  Permutation p is ``torch.randperm(N, generator=g,
    device=...)`` from one generator seeded with ``seed``, drawn one at a time in order.  ``return_sims=True`` keeps the
    (D, P) simulated values.  This permutes the spot labels against a fixed graph, which is PySAL's definition; squidpy
    shuffles the rows of its adjacency matrix instead -- both are null models of exchangeable spots, but the numbers differ
    draw by draw.  The smallest attainable p-value is 1 / (P + 1).  The comparisons I_pi >= I are exact for integer-valued
    data (counts), ties included; for other values a mathematical tie may fall either way in the last bit.

    ``mode="geary"`` scores Geary's C instead, squidpy's ``spatial_autocorr(mode="geary")``: squared differences along the
    edges over the variance, 1 in expectation and BELOW 1 for positive autocorrelation, more sensitive to local structure
    than I.  It returns a ``GeneGeary`` -- ``z`` = (C - 1) / sqrt(variance), negative for positive autocorrelation -- or with
    permutations a ``GeneGearyPerm``, whose ``pval_less`` is the one for positive autocorrelation
    (``ops.gene_spatial_stats_sparse`` / ``ops.spatial_stats``, ``ops.gene_autocorr_perm_sparse`` /
    ``ops.autocorr_perm_rows``).  ``assumption="randomisation"`` replaces the normality moments, which depend on the graph
    alone, by the randomisation moments of Cliff & Ord (PySAL's ``VI_rand`` / ``VC_rand``): ``variance`` and ``z`` become
    (D,) tensors that depend on each gene's kurtosis (``gene_kurtosis``).  They are the exact mean and variance of the
    statistic over all N! relabellings of the spots -- what the permutation null samples -- and for counts, which are far
    from normal, the ones to use; N >= 4 is needed.  Both defaults give the call without these keywords, bit for bit."""
    import numpy as np
    from . import ops
    from .likelihoods import SparseCounts, SparseExpression, TransposedCounts
    who = "gene_autocorr"
    if mode not in ("moran", "geary"):
        raise ValueError(f"{who}: mode={mode!r} unknown ('moran', 'geary')")
    if assumption not in ("normality", "randomisation"):
        raise ValueError(f"{who}: assumption={assumption!r} unknown ('normality', 'randomisation')")
    if isinstance(values, TransposedCounts):
        raise TypeError(f"{who}: values is the .T (obs x feat) of a SparseCounts; pass the SparseCounts itself (genes x spots)")
    sparse = isinstance(values, (SparseCounts, SparseExpression))
    if sparse:
        ops._whole_values(values, who)
    elif not isinstance(values, torch.Tensor):
        raise TypeError(f"{who}: a SparseCounts, a SparseExpression or a dense (D, N) tensor expected, got {type(values).__name__}")
    elif values.dim() != 2 or not values.is_floating_point():
        raise ValueError(f"{who}: a dense (D, N) floating-point tensor expected, got {tuple(values.shape)} of {values.dtype}")
    D, N = values.shape
    dev = values.device
    if assumption == "randomisation" and N < 4:
        raise ValueError(f"{who}: assumption='randomisation' needs N >= 4 spots, got {N}")
    permute = n_perms is not None or perms is not None
    if permute:
        P, perms = _autocorr_perms(who, N, n_perms, perms)
    if graph is not None:
        nbr = graph.detach() if isinstance(graph, torch.Tensor) else torch.as_tensor(np.asarray(graph))
        if nbr.dim() != 2 or nbr.shape[0] != N or nbr.dtype.is_floating_point or nbr.dtype == torch.bool:
            raise ValueError(f"{who}: graph must be an ({N}, K) integer table")
        nbr = nbr.to(device=dev, dtype=torch.int64)
    else:
        if coords is None:
            raise ValueError(f"{who}: coords (N, d) or graph= (N, K) needed")
        X = coords.detach() if isinstance(coords, torch.Tensor) else torch.as_tensor(np.asarray(coords))
        if X.dim() != 2 or X.shape[0] != N:
            raise ValueError(f"{who}: coords {tuple(X.shape)} for {N} spots ((N, d) expected)")
        if X.dtype not in (torch.float32, torch.float64):
            X = X.double()
        X = X.to(dev)
        if not bool(torch.isfinite(X).all()):
            raise ValueError(f"{who}: coords hold a non-finite value")
        nbr = ops.spatial_knn(X, int(n_neighs))
    K = int(nbr.shape[1])
    if not 1 <= K <= 32 or K >= N:
        raise ValueError(f"{who}: {K} neighbours of {N} spots unsupported (1 <= K <= 32, K < N)")
    if permute and perms is None:
        g = torch.Generator(device=dev)
        g.manual_seed(int(seed))
        perms = torch.empty((P, N), dtype=torch.int32, device=dev)
        for p in range(P):
            perms[p] = torch.randperm(N, generator=g, device=dev)
    if mode == "geary" or assumption == "randomisation":
        return _gene_autocorr_stats(values, sparse, nbr, perms if permute else None, return_sims, mode, assumption)
    if sparse and permute:
        r = ops.gene_morans_perm_sparse(values, nbr, perms, return_sims=return_sims)
        I = r.I
    elif sparse:
        I = ops.gene_morans_i_sparse(values, nbr)
    else:
        V = values.detach()
        I = ops.morans_i((V if V.dtype in (torch.float32, torch.float64) else V.float()).T.contiguous(), nbr)
        if permute:
            r = ops.morans_perm_rows(V.float(), nbr, perms, return_sims=return_sims)
    expected, variance = _moran_moments(nbr)
    base = GeneAutocorr(I, expected, variance, (I - expected) / torch.sqrt(variance))
    if not permute:
        return base
    return GeneAutocorrPerm(*base, *_perm_fields(I, r, P))


def _perm_fields(I, r, P):
    """The fields of ``GeneAutocorrPerm`` / ``GeneGearyPerm`` after ``z``, from the observed statistic and the permutation
    entry's result."""
    nan = torch.isnan(I) | torch.isnan(r.sim_mean)
    quiet = torch.full_like(I, float("nan"))
    n_ge, n_le = (torch.where(nan, torch.zeros_like(n), n) for n in (r.n_ge, r.n_le))
    pg, pl = (torch.where(nan, quiet, (n.double() + 1.0) / (P + 1.0)) for n in (n_ge, n_le))
    mean_sim = torch.where(nan, quiet, r.sim_mean)
    var_sim = torch.where(nan, quiet, r.sim_m2 / P)
    z_sim = torch.where(var_sim > 0, (I - mean_sim) / torch.sqrt(var_sim), quiet)
    pval_z = 0.5 * torch.erfc(z_sim.abs() / 2.0 ** 0.5)
    return P, n_ge, n_le, pg, pl, torch.minimum(pg, pl), mean_sim, var_sim, z_sim, pval_z, r.sims


def _gene_autocorr_stats(values, sparse, nbr, perms, return_sims, mode, assumption):
    """``gene_autocorr`` beyond its defaults: Geary's C and / or the randomisation moments, through the entries that give C
    and the kurtosis beside I."""
    from . import ops
    if sparse:
        st = ops.gene_spatial_stats_sparse(values, nbr)
    else:
        V = values.detach()
        st = ops.spatial_stats((V if V.dtype in (torch.float32, torch.float64) else V.float()).T.contiguous(), nbr)
    stat = st.C if mode == "geary" else st.I
    if perms is not None and sparse:
        r = ops.gene_autocorr_perm_sparse(values, nbr, perms, stat=mode, return_sims=return_sims)
        stat = r.value                                   # st's, bit for bit
    elif perms is not None:
        r = ops.autocorr_perm_rows(values.detach().float(), nbr, perms, stat=mode, return_sims=return_sims)
    m = _autocorr_moments(nbr, st.kurtosis if assumption == "randomisation" else None)
    key = ("VC" if mode == "geary" else "VI") + ("_rand" if assumption == "randomisation" else "_norm")
    expected, variance = m["EC" if mode == "geary" else "EI"], m[key]
    kinds = (GeneGeary, GeneGearyPerm) if mode == "geary" else (GeneAutocorr, GeneAutocorrPerm)
    base = kinds[0](stat, expected, variance, (stat - expected) / torch.sqrt(variance))
    if perms is None:
        return base
    return kinds[1](*base, *_perm_fields(stat, r, int(perms.shape[0])))


def fdr_bh(p):
    """Benjamini-Hochberg adjusted p-values of a 1-D tensor (the FDR correction squidpy and statsmodels put on top of
    ``pval_sim``): with the m entries that are not NaN sorted increasingly, q_(i) = min_{j >= i} min(1, m p_(j) / j) -- the
    step-up rule as a running minimum from the largest p.  NaN entries are not counted in m and stay NaN.  Pure torch, on the
    tensor's device; returns fp64."""
    if not isinstance(p, torch.Tensor) or p.dim() != 1:
        raise ValueError("fdr_bh: a 1-D tensor of p-values expected")
    p = p.detach().to(torch.float64)
    out = torch.full_like(p, float("nan"))
    ok = ~torch.isnan(p)
    m = int(ok.sum())
    if m == 0:
        return out
    vals, order = torch.sort(p[ok], descending=True, stable=True)
    rank = torch.arange(m, 0, -1, dtype=torch.float64, device=p.device)
    q = torch.cummin(vals * m / rank, dim=0).values.clamp(max=1.0)
    adj = torch.empty_like(q)
    adj[order] = q
    out[ok] = adj
    return out


def _rank_order(score, nfeat=None):
    """Indices of ``score`` in decreasing order, NaN last, equal values in index order (the rules of
    ``dims_autocorr(sort=True)``), cut to the first ``nfeat``."""
    nan = torch.isnan(score)
    order = torch.argsort(torch.where(nan, torch.full_like(score, float("inf")), -score), stable=True)
    last = nan[order]                                  # NaN after everything else, -inf included, whatever the device's
    order = torch.cat([order[~last], order[last]])     # sort makes of a NaN key
    if nfeat is not None:
        if not 1 <= int(nfeat) <= score.numel():
            raise ValueError(f"rank_genes: nfeat={nfeat} out of {score.numel()} genes")
        order = order[:int(nfeat)]
    return order


def rank_genes(counts, by="deviance", *, coords=None, nfeat=None, **kw):
    """``(order, score)`` of the genes of a whole ``SparseCounts``: ``order`` int64 (D,), or (nfeat,), in decreasing score
    (NaN last, ties in gene order), ``score`` fp64 aligned with it; ``counts.select_genes(order)`` is then the reference's
    ``ad[:, :nfeat]`` of a data set sorted by importance.  ``by``: "deviance" (``gene_deviance``, Poisson),
    "binomial_deviance", "moran" (``gene_autocorr`` of ``log_normalize(counts, center=False)`` over ``coords``), "geary"
    (1 - C of the same values, ``gene_autocorr(mode="geary")``: larger is more autocorrelated, as with every score), or
    "overdispersion" (``gene_dispersion(counts).lr``, the likelihood-ratio statistic of NB against Poisson), or "gp"
    (``gene_spatial_gp(log_normalize(counts), coords).lr``, the sparse-GP likelihood ratio against no spatial term;
    ``size_factors=`` goes to ``log_normalize``).  Extra keywords go to the scorer."""
    if by == "deviance":
        score = gene_deviance(counts, "poisson", **kw)
    elif by == "binomial_deviance":
        score = gene_deviance(counts, "binomial", **kw)
    elif by == "moran":
        _whole_counts_only(counts, "rank_genes")
        if coords is None and kw.get("graph") is None:
            raise ValueError("rank_genes: by='moran' needs coords (or graph=)")
        score = gene_autocorr(log_normalize(counts, center=False), coords, **kw).I
    elif by == "geary":
        _whole_counts_only(counts, "rank_genes")
        if coords is None and kw.get("graph") is None:
            raise ValueError("rank_genes: by='geary' needs coords (or graph=)")
        score = 1.0 - gene_autocorr(log_normalize(counts, center=False), coords, mode="geary", **kw).C
    elif by == "overdispersion":
        score = gene_dispersion(counts, **kw).lr
    elif by == "gp":
        _whole_counts_only(counts, "rank_genes")
        if coords is None:
            raise ValueError("rank_genes: by='gp' needs coords")
        score = gene_spatial_gp(log_normalize(counts, kw.pop("size_factors", None)), coords, **kw).lr
    else:
        raise ValueError(f"rank_genes: by={by!r} unknown ('deviance', 'binomial_deviance', 'moran', 'geary', 'overdispersion', 'gp')")
    order = _rank_order(score, nfeat)
    return order, score[order]


def train_val_split(X, y, train_frac=0.95, sz="constant"):
    """The train / validation split of the reference's ``anndata_to_train_val`` (utilities.py:192-230) in this project's
    orientation: ``y`` is the (D genes, N spots) count matrix, a dense tensor or a whole ``SparseCounts``, ``X`` the (N, d)
    coordinates.  The first ``round(train_frac * N)`` spots train, the rest are held out (the spots are assumed
    pre-shuffled).  ``sz``: "constant" (ones), "mean" (a spot's mean count) or "scanpy" (spot totals over their median,
    per split as the reference computes it).

    Returns ``(Dtr, Dval)``, dicts with ``X`` (rows of X, not rescaled here), ``y`` (D, n), ``sz`` (n,) and ``idx`` (the
    spots' positions in the input); ``Dval`` is None when nothing is held out.  Of a ``SparseCounts`` each split's ``y`` is
    a whole ``SparseCounts`` again (built once from the filtered non-zeros), so the training loops can take ``y[:, idx]``
    of it; the held-out ``sz`` are the explicit size factors ``model.deviance(..., V=)`` wants."""
    from .likelihoods import SparseCounts
    if sz not in ("constant", "mean", "scanpy"):
        raise ValueError("unrecognized size factors 'sz'")
    sparse = isinstance(y, SparseCounts)
    if sparse and y.base is not y:
        raise TypeError("train_val_split: y is a view y[:, idx]; split the SparseCounts itself")
    if not sparse:
        y = torch.as_tensor(y)
        if y.dim() != 2:
            raise ValueError(f"train_val_split: a (genes, spots) matrix expected, got {y.dim()} dimensions")
    D, N = y.shape
    if X.shape[0] != N:
        raise ValueError(f"train_val_split: {X.shape[0]} rows of X for {N} spots (y is genes x spots)")
    Ntr = round(train_frac * N)
    if not 1 <= Ntr <= N:
        raise ValueError(f"train_val_split: train_frac = {train_frac} leaves {Ntr} of {N} spots to train on")
    if sparse:
        gene, spot, val = y.col_gene.long(), y._spots(), y.col_val

    def part(lo, hi):
        n = hi - lo
        if sparse:
            keep = (spot >= lo) & (spot < hi)
            yp = SparseCounts(torch.sparse_coo_tensor(torch.stack([gene[keep], spot[keep] - lo]), val[keep], (D, n)))
            dtype, device = torch.float32, y.device
        else:
            yp = y[:, lo:hi]
            dtype, device = (y.dtype if y.is_floating_point() else torch.float32), y.device
        if sz == "constant":
            s = torch.ones(n, dtype=dtype, device=device)
        else:
            Yp = yp.T if sparse else yp.T.cpu().numpy()            # obs x feat, as the reference holds it
            s = scanpy_sizefactors(Yp) if sz == "scanpy" else _spot_totals(Yp) / D
            s = torch.as_tensor(s).reshape(-1).to(device=device, dtype=dtype)
        return dict(X=X[lo:hi], y=yp, sz=s, idx=torch.arange(lo, hi))

    return part(0, Ntr), (part(Ntr, N) if Ntr < N else None)


def rescale_spatial_coords(X, box_side=4):
    """The coordinates X (N,d) shifted to a zero minimum, scaled by ``box_side`` over the geometric mean of the
    extents -- the aspect ratio is kept and the bounding box gets the volume ``box_side ** d`` -- and centred at their
    mean; ``box_side=4`` puts them roughly in (-2, 2) (reference utilities.py:177-190).  The arithmetic is the
    reference's, in X's own floating dtype.  Unlike the reference, which shifts and scales the caller's array in place
    before it returns the centred copy, the caller's array is never modified; the returned values are the same."""
    import numpy as np
    X = np.array(X, copy=True)
    if not np.issubdtype(X.dtype, np.floating):
        X = X.astype(np.float64)
    X -= X.min(axis=0)
    X *= box_side / np.exp(np.mean(np.log(X.max(axis=0))))
    return X - X.mean(axis=0)


def smooth_spatial_factors(F, Z, X=None):
    """Starting values of an NSF model at its inducing points from factors at the spots (reference utilities.py:50-68;
    ``regularized_nmf`` gives F (N,L) on the log scale, ``gp.mu`` is U.T).  Returns numpy ``(U (M,L), beta0 (L,),
    beta (L,d))``:

    ``U``: for each row of Z (M,d) the uniform mean of F over the ``K = max(2, ceil(N / M))`` spots of X (N,d) nearest to
    it -- sklearn's ``KNeighborsRegressor(n_neighbors=K).fit(X, F).predict(Z)`` -- as one HIP selection
    (``ops.knn_mean``, gpz_knn_mean) on the GPU of the tensor arguments, or on the current GPU for numpy / host inputs.
    The K smallest (fp64 squared distance, index) keys are taken: sklearn's set wherever no exact distance tie falls on
    the K-th place (there its tree's visit order decides, here the lower index) -- the one place the result can differ
    from the reference.  ``beta0``, ``beta``: intercept and coefficients of the least-squares trend of F on X, sklearn's
    ``LinearRegression().fit(X, F)``: the centred normal equations are formed in fp64 on the device and their
    minimum-norm solution (``numpy.linalg.lstsq``) is taken on the host, which is sklearn's answer for rank-deficient
    (e.g. collinear) coordinates too.

    ``X=None``: ``beta0 = F.mean(0)``, U is that mean tiled M times and beta is None -- on the host, no GPU needed.

    F, Z, X: numpy arrays or torch tensors, host or CUDA.  Everything is computed in fp64 and rounded at the end:
    float32 F gives float32 outputs (as the reference does), anything else float64.  ValueError, before anything touches
    a GPU: F not (N,L), Z or X not 2-D, row counts of F and X that differ, coordinate dimensions that differ or lie
    outside 1..4, L > 256, N < K; after one device check: a non-finite coordinate or factor."""
    import math
    import numpy as np

    def as_tensor(a):
        return a.detach() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))

    Ft, Zt = as_tensor(F), as_tensor(Z)
    if Ft.dim() != 2:
        raise ValueError(f"smooth_spatial_factors: F must be (N, L), got shape {tuple(Ft.shape)}")
    if Zt.dim() != 2:
        raise ValueError(f"smooth_spatial_factors: Z must be (M, d), got shape {tuple(Zt.shape)}")
    N, L = Ft.shape
    M = Zt.shape[0]
    out = np.float32 if Ft.dtype == torch.float32 else np.float64
    if X is None:
        beta0 = Ft.cpu().numpy().astype(np.float64).mean(axis=0)
        return np.tile(beta0, [M, 1]).astype(out), beta0.astype(out), None
    Xt = as_tensor(X)
    if Xt.dim() != 2:
        raise ValueError(f"smooth_spatial_factors: X must be (N, d), got shape {tuple(Xt.shape)}")
    if Xt.shape[0] != N:
        raise ValueError(f"smooth_spatial_factors: {N} rows of F but {Xt.shape[0]} of X")
    d = Xt.shape[1]
    if Zt.shape[1] != d:
        raise ValueError(f"smooth_spatial_factors: X has {d} coordinates per point, Z {Zt.shape[1]}")
    if not 1 <= d <= 4:
        raise ValueError(f"smooth_spatial_factors: coordinates of dimension {d} unsupported (1..4)")
    if not 1 <= L <= 256:
        raise ValueError(f"smooth_spatial_factors: L={L} unsupported (1..256)")
    if M < 1:
        raise ValueError("smooth_spatial_factors: Z holds no inducing point")
    K = max(2, math.ceil(N / M))
    if N < K:
        raise ValueError(f"smooth_spatial_factors: {N} observations, at least n_neighbors={K} needed")
    from . import ops
    dev = next((t.device for t in (Ft, Zt, Xt) if t.is_cuda), None)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    ct = torch.float32 if Xt.dtype == Zt.dtype == torch.float32 else torch.float64
    Xt, Zt = Xt.to(device=dev, dtype=ct), Zt.to(device=dev, dtype=ct)
    Ft = Ft.to(device=dev, dtype=torch.float32 if Ft.dtype == torch.float32 else torch.float64)
    if not bool(torch.isfinite(Xt).all() & torch.isfinite(Zt).all() & torch.isfinite(Ft).all()):
        raise ValueError("smooth_spatial_factors: F, Z or X holds a non-finite value")
    U = ops.knn_mean(Xt, Ft, Zt, K).cpu().numpy()
    Xd, Fd = Xt.double(), Ft.double()
    mx, mf = Xd.mean(dim=0), Fd.mean(dim=0)
    Xc, Fc = Xd - mx, Fd - mf
    G, C = (Xc.t() @ Xc).cpu().numpy(), (Xc.t() @ Fc).cpu().numpy()
    beta = np.linalg.lstsq(G, C, rcond=None)[0].T
    beta0 = mf.cpu().numpy() - beta @ mx.cpu().numpy()
    return U.astype(out), beta0.astype(out), beta.astype(out)


KMEANS_BLOCK = 16     # Lloyd iterations enqueued between two reads of the device's stop record


def kmeans_inducing_points(X, M, *, init="k-means++", max_iter=300, tol=1e-4, random_state=None, return_info=False):
    """The (M,d) k-means centres of the spots X (N,d) -- the usual inducing points Z of a sparse GP, and what the
    notebooks get from ``KMeans(n_clusters=M).fit(X).cluster_centers_`` -- by k-means++ seeding and Lloyd's iterations
    in HIP (``ops.kmeans_seed`` / ``kmeans_lloyd`` / ``kmeans_assign``) on X's GPU, or on the current GPU for numpy / host
    inputs.  It is sklearn's ``KMeans(n_clusters=M, n_init=1, algorithm="lloyd", max_iter=max_iter, tol=tol)``; no sklearn
    is imported.

    sklearn-exact: Lloyd from a given start (``init`` an (M,d) array) -- the same labels and number of iterations, centres
    and inertia to fp64 rounding, wherever no point lies within rounding of two centres.  The distance is fp64, each
    (x_k - c_k)^2 rounded and added in coordinate order; ties go to the lower centre index; centres are fp64 means; the stop
    is by repeated labels, else by shift <= tol * mean(var(X, axis=0)) (fp64, population form), else at ``max_iter``.
    Defined here: (1) the random stream.  ``init="k-means++"`` is sklearn's greedy ``_kmeans_plusplus`` (2 + floor(ln M)
    trials per centre) driven by ``np.random.default_rng(random_state).random((M, T))``, and ``init="random"`` takes the rows
    ``np.random.default_rng(random_state).choice(N, M, replace=False)``: a seeded result therefore DIFFERS from sklearn's
    for the same ``random_state`` (its choices hang on float32 GEMM-form distances and numpy's legacy generator); it is the
    same algorithm and the same quality.  (2) the pairing of several empty clusters with the points relocated to them: the
    farthest point goes to the lowest empty cluster (sklearn's pairing is ``argpartition``'s, which is unspecified; for one
    empty cluster the choice is sklearn's).  A cluster left without a member stays at its old centre.  Every sum runs in a
    fixed order without floating-point atomics: two calls on the same input agree bit for bit.

    Limits: 1 <= d <= 4, 1 <= M <= N < 2**31, dense X, no sample weights, ``n_init = 1``.

    X: numpy array or torch tensor (host or CUDA), float32 or float64 (anything else is taken as float64).  Returns the
    centres in X's dtype: numpy for numpy, a tensor on X's device for a tensor.  ``return_info=True`` adds a dict:
    ``labels`` (N,) int64, ``inertia`` (float), ``n_iter`` (int), ``converged`` ("labels", "tol" or False),
    ``seed_indices`` ((M,) int64 of the rows the start was taken from, None for an array ``init``) -- labels and
    seed_indices of X's kind.  ValueError, before anything touches a GPU: X not (N,d), d outside 1..4, M outside 1..N,
    an unknown ``init`` string or an ``init`` array that is not (M,d), ``max_iter < 1``, ``tol < 0``, a non-finite ``init``,
    a non-finite X (checked where X lives: on the host for host input, by one device reduction for a CUDA tensor, before
    any k-means launch)."""
    import math
    import numpy as np

    who = "kmeans_inducing_points"
    is_tensor = isinstance(X, torch.Tensor)
    Xt = X.detach() if is_tensor else torch.as_tensor(np.asarray(X))
    if Xt.dim() != 2:
        raise ValueError(f"{who}: X must be (N, d), got shape {tuple(Xt.shape)}")
    N, d = Xt.shape
    if not 1 <= d <= 4:
        raise ValueError(f"{who}: coordinates of dimension {d} unsupported (1..4)")
    if isinstance(M, bool) or not isinstance(M, (int, np.integer)):
        raise ValueError(f"{who}: M must be an integer, got {M!r}")
    M = int(M)
    if not 1 <= M <= N:
        raise ValueError(f"{who}: M={M} outside 1..N={N}")
    if N >= 2 ** 31:
        raise ValueError(f"{who}: N={N} unsupported (N < 2**31)")
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError(f"{who}: max_iter={max_iter!r} must be an integer >= 1")
    if not (isinstance(tol, (int, float, np.floating, np.integer)) and tol >= 0):
        raise ValueError(f"{who}: tol={tol!r} must be a number >= 0")
    C0 = None
    if isinstance(init, str):
        if init not in ("k-means++", "random"):
            raise ValueError(f"{who}: unknown init {init!r} ('k-means++', 'random' or an (M, d) array)")
    else:
        C0 = init.detach() if isinstance(init, torch.Tensor) else torch.as_tensor(np.asarray(init))
        if tuple(C0.shape) != (M, d):
            raise ValueError(f"{who}: init must be ({M}, {d}), got shape {tuple(C0.shape)}")
        C0 = torch.as_tensor(C0.cpu().numpy().astype(np.float64))
        if not bool(np.isfinite(C0.numpy()).all()):
            raise ValueError(f"{who}: init holds a non-finite value")
    out_dtype = Xt.dtype if Xt.dtype in (torch.float32, torch.float64) else torch.float64

    if Xt.is_floating_point() and not bool(torch.isfinite(Xt).all()):       # (on X's own device: the host for host input)
        raise ValueError(f"{who}: X holds a non-finite value")

    from . import ops
    dev = Xt.device if Xt.is_cuda else torch.device("cuda", torch.cuda.current_device())
    Xd = Xt.to(device=dev, dtype=out_dtype).contiguous()

    seed_idx = None
    if C0 is not None:
        C = C0.to(dev).contiguous()
    elif init == "random":
        seed_idx = torch.as_tensor(np.random.default_rng(random_state).choice(N, M, replace=False).astype(np.int64)).to(dev)
        C = Xd[seed_idx].double().contiguous()
    else:
        T = 2 + int(math.log(M))
        u = torch.as_tensor(np.random.default_rng(random_state).random((M, T))).to(dev)
        seed_idx, C = ops.kmeans_seed(Xd, M, u)
    tol_abs = float(tol) * float(Xd.double().var(dim=0, unbiased=False).mean())
    labels = torch.full((N,), -1, dtype=torch.int32, device=dev)
    state = ops.kmeans_state(dev)
    done, stop = 0, 0
    while done < max_iter and stop == 0:
        ops.kmeans_lloyd(Xd, C, labels, state, tol_abs, min(KMEANS_BLOCK, max_iter - done))
        host = state.cpu()
        done, stop = int(host[0]), int(host[1])
    if stop == 1:
        _, inertia = ops.kmeans_assign(Xd, C, labels)
    else:
        labels, inertia = ops.kmeans_assign(Xd, C)
    centres = C.to(out_dtype)
    if not is_tensor:
        centres = centres.cpu().numpy()
    elif not Xt.is_cuda:
        centres = centres.cpu()
    if not return_info:
        return centres

    def like_x(t):
        t = t.to(torch.int64)
        return t.cpu().numpy() if not is_tensor else (t if Xt.is_cuda else t.cpu())

    info = dict(labels=like_x(labels), inertia=float(inertia), n_iter=done, converged={1: "labels", 2: "tol"}.get(stop, False),
                seed_indices=None if seed_idx is None else like_x(seed_idx))
    return centres, info


def project_factors_to_inducing(kernel, Z, X, F, *, jitter=1e-5, whitened=False, kzz_jitter=0.0, return_info=False):
    """Start for ``gp.mu`` by kernel least squares: per latent ``alpha = (K_zx K_xz + jitter I)^-1 K_zx f``, so that
    ``K_xz alpha ~ f``, and ``mu = K_zz alpha`` -- what Slideseqv2_estimate_lengthscales.ipynb (``build_model_scracth``:
    ``L1 = cholesky(add_jitter(Kzx @ Kxz, 1e-5)); alpha = cholesky_solve(Kzx @ F, L1); mu = Kzz @ alpha``) and
    NSF_Hybrid_benchmark.ipynb (``torch.pinverse(Kzx @ Kxz)``) compose by hand from a materialised ``kernel(Z, X)``.  Here
    the Gram matrix and the right-hand sides come from one HIP pass over X (``ops.kernel_gram``, gpz_kernel_gram) that never
    stores K_zx and adds in a fixed order; the factorisation (``ops.cholesky``) and the solves are fp64.

    ``kernel``: ``RBF``, ``NSF_RBF``, ``batched_RBF``, ``batched_Matern12`` / ``32`` / ``52`` of this package (a multi-group
    kernel or a user-defined ``covariance`` raises NotImplementedError).  Z (M,d), X (N,d), F (L,N): one row per latent, the
    notebooks' ``factors.T[:L]``.  A kernel with per-latent parameters pairs latent l with row l (their counts must
    agree); a scalar-parameter kernel has one Gram matrix, factored once, for all L rows.

    Returns ``mu`` (L,M): ``whitened=False`` (for ``SVGP``) ``K_zz alpha`` with K_zz as the kernel gives it, without jitter,
    as in the notebook; ``whitened=True`` (for ``WSVGP``) ``Lz^T alpha`` with ``Lz = chol(K_zz + kzz_jitter I)`` -- pass
    ``gp.jitter``.  ``return_info=True`` adds a dict: ``alpha`` (L,M), ``gram_diag_min`` / ``gram_diag_max`` (floats, of
    the factored matrix, jitter included) and ``residual`` (L,) = ||K_xz alpha - f||^2 / ||f||^2, evaluated without a second
    pass over X as ``(f.f - 2 alpha.b + alpha.G alpha) / f.f`` in fp64 with the jitter taken out of G: a difference of
    numbers near f.f, so a nearly exact fit (residual below about 1e-6 on the fp32 path, 1e-12 in fp64) loses its digits and
    may come out slightly negative.

    Precision: fp32 covariance entries (the bits ``kernel(Z, X)`` holds) and fp32 products inside one N-split when Z, X and
    the kernel's parameters are all float32, fp64 otherwise; Gram matrix, right-hand side, factorisation and solves are
    fp64 in both cases.  On the fp32 path an entry of the Gram matrix is good to about 1e-6 of its largest diagonal entry:
    where K_zx K_xz is nearly singular (inducing points drawn from the spots, a lengthscale above their spacing) a jitter
    below that cannot keep it positive definite -- pass float64 coordinates, which cost the fp64 rate of the one pass.
    Repeated calls agree bit for bit.  Inputs are numpy arrays or torch tensors, host or CUDA; the
    work runs on the GPU of the first CUDA argument, else on the current one.  ``mu`` and ``alpha`` are of F's kind (numpy,
    or a tensor on F's device), float32 for float32 F, else float64.

    ValueError, before anything touches a GPU: wrong ranks, row counts that differ, d outside 1..4, an L mismatch,
    ``jitter < 0`` or ``kzz_jitter < 0``, N = 0 or M = 0, M > 8192, a non-finite value in a host input (a CUDA input is
    checked by one device reduction before any launch).  torch.linalg.LinAlgError: ``K_zx K_xz + jitter I`` (or, whitened,
    ``K_zz + kzz_jitter I``) is not positive definite."""
    import numpy as np
    from . import kernels as _k

    who = "project_factors_to_inducing"
    if isinstance(kernel, _k._MGGPMixin):
        raise NotImplementedError(f"{who}: multi-group kernels ({type(kernel).__name__}) are not supported")
    if not isinstance(kernel, _k._HipKernel):
        raise TypeError(f"{who}: {type(kernel).__name__} is not a kernel of gpzoo.kernels")
    kernel._check_covariance()

    def as_tensor(a):
        return a.detach() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))

    f_is_tensor = isinstance(F, torch.Tensor)
    Zt, Xt, Ft = as_tensor(Z), as_tensor(X), as_tensor(F)
    for name, t, want in (("Z", Zt, "(M, d)"), ("X", Xt, "(N, d)"), ("F", Ft, "(L, N)")):
        if t.dim() != 2:
            raise ValueError(f"{who}: {name} must be {want}, got shape {tuple(t.shape)}")
    (M, d), N, L = Zt.shape, Xt.shape[0], Ft.shape[0]
    if Xt.shape[1] != d:
        raise ValueError(f"{who}: X has {Xt.shape[1]} coordinates per point, Z {d}")
    if not 1 <= d <= 4:
        raise ValueError(f"{who}: coordinates of dimension {d} unsupported (1..4)")
    if Ft.shape[1] != N:
        raise ValueError(f"{who}: {N} rows of X but {Ft.shape[1]} columns of F")
    if N < 1 or M < 1 or L < 1:
        raise ValueError(f"{who}: nothing to project (N={N}, M={M}, L={L})")
    if M > 8192 or N >= 2 ** 31:
        raise ValueError(f"{who}: M={M}, N={N} unsupported (M <= 8192, N < 2**31)")
    for name, v in (("jitter", jitter), ("kzz_jitter", kzz_jitter)):
        if not (isinstance(v, (int, float, np.floating, np.integer)) and v >= 0):
            raise ValueError(f"{who}: {name}={v!r} must be a number >= 0")
    spec = kernel._spec()
    if spec.batched and spec.L != L:
        raise ValueError(f"{who}: the kernel has parameters for {spec.L} latents, F has {L} rows")
    floats = [t if t.is_floating_point() else t.double() for t in (Zt, Xt, Ft, spec.sigma, spec.lengthscale)]
    finite = [torch.isfinite(t).all() for t in floats]
    host = [f for f in finite if not f.is_cuda]
    if host and not bool(torch.stack(host).all()):
        raise ValueError(f"{who}: Z, X, F or a kernel parameter holds a non-finite value")
    dev_flags = [f for f in finite if f.is_cuda]

    from . import ops
    Zt, Xt, Ft, sig, ell = floats
    dev = next((t.device for t in (Ft, Zt, Xt, sig) if t.is_cuda), None)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev_flags and not bool(torch.stack([f.to(dev) for f in dev_flags]).all()):
        raise ValueError(f"{who}: Z, X, F or a kernel parameter holds a non-finite value")
    ct = torch.float32 if all(t.dtype == torch.float32 for t in (Zt, Xt, sig, ell)) else torch.float64
    out_dtype = torch.float32 if Ft.dtype == torch.float32 else torch.float64
    Zd, Xd = Zt.to(device=dev, dtype=ct).contiguous(), Xt.to(device=dev, dtype=ct).contiguous()
    Fd = Ft.to(device=dev, dtype=torch.float64).contiguous()
    spec = ops.KernelSpec(spec.kind, sig.to(device=dev, dtype=ct).contiguous(), ell.to(device=dev, dtype=ct).contiguous(),
                          spec.batched)

    G, b = ops.kernel_gram(spec, Zd, Xd, Fd.to(ct), float(jitter))          # (n, M, M), (n, R, M) fp64
    Lg = ops.cholesky(G)

    def solve(Lc, rhs):          # (Lc Lc^T)^-1 rhs by two triangular solves; rhs (n, M, 1)
        y = ops.solve_triangular_lower(Lc, rhs.contiguous())
        return torch.linalg.solve_triangular(Lc.transpose(-1, -2), y, upper=True)[:, :, 0]

    Kzz = ops.kfill(spec, Zd, Zd).double()                                    # (L, M, M) or (M, M)
    if whitened:
        eye = torch.eye(M, dtype=torch.float64, device=dev)
        T = torch.tril(ops.cholesky(Kzz + float(kzz_jitter) * eye)).transpose(-1, -2)
    else:
        T = Kzz
    if spec.batched:
        alpha = solve(Lg, b.transpose(-1, -2))                                # (L, M)
        mu = (T * alpha[:, None, :]).sum(-1)
    else:
        # one factorisation, then row by row: row l of a call with L rows is computed exactly as a call with that row alone
        alpha = torch.cat([solve(Lg, b[:, l, :, None]) for l in range(L)])
        mu = torch.stack([(T * alpha[l][None, :]).sum(-1) for l in range(L)])

    def like_f(t):
        t = t.to(out_dtype)
        if not f_is_tensor:
            return t.cpu().numpy()
        return t if Ft.is_cuda else t.cpu()

    if not return_info:
        return like_f(mu)
    diag = torch.diagonal(G, dim1=-2, dim2=-1)
    ff = (Fd * Fd).sum(dim=1)
    bL = b[:, 0, :] if spec.batched else b[0]                                 # (L, M)
    Ga = (G @ alpha[:, :, None])[:, :, 0] if spec.batched else (G[0] @ alpha.t()).t()
    quad = (alpha * Ga).sum(dim=1) - float(jitter) * (alpha * alpha).sum(dim=1)
    residual = (ff - 2.0 * (alpha * bL).sum(dim=1) + quad) / ff
    info = dict(alpha=like_f(alpha), gram_diag_min=float(diag.min()), gram_diag_max=float(diag.max()),
                residual=like_f(residual))
    return like_f(mu), info


# Host-side data preparation of the reference's utilities module (AnnData conversion, plotting, ...) is outside the
# accelerated path and not rebuilt here.  The names resolve so that
# ``from gpzoo.utilities import train_hybrid, anndata_to_train_val`` -- the notebooks' import lines -- keep
# working; calling one says where it lives.
_NOT_REBUILT = ("build_group_distances", "anndata_to_train_val", "plot_factors")


def __getattr__(name):
    if name in _NOT_REBUILT:
        def _missing(*args, **kwargs):
            raise NotImplementedError(
                f"gpzoo.utilities.{name} is host-side data preparation outside the MI355X hot path and is not "
                f"rebuilt in gpzoo_amd; use the reference package's function of the same name for it")
        _missing.__name__ = name
        return _missing
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
