"""Gaussian likelihood wrappers with the gpzoo.likelihoods class API.

Thin consumers of the hot path's outputs (they stay torch):
``forward`` calls the GP once -- one fused HIP pass -- and wraps the result in
torch distributions exactly like reference likelihoods.py:7-36.  The Poisson
factor models (SURVEY §8f "next" #2) follow below: same classes and return tuples
as the reference, plus ``expected_loglik`` -- the fused fp32 training-step form
(``gpz_poisson_nsf``; fp64 models are evaluated in fp32 there and cast back).
``likelihood="nb"`` on any of the count models swaps the Poisson noise for a negative binomial with one inverse
dispersion per gene (the nsf paper's ``lik="nb"``): ``pY`` is a torch NegativeBinomial and ``expected_loglik`` runs
the fused ``gpz_nb_nsf`` step.
``RSF`` and ``FA`` at the end are the Gaussian factor models for normalised, real-valued expression: real loadings, an
intercept and a noise level per gene, and an exact ``expected_loglik`` through the fused ``gpz_gaussian_fa`` step -- or,
for a ``SparseExpression`` (centred log-normalised counts held as the stored entries minus a per-gene offset,
``utilities.log_normalize``), through ``gpz_gaussian_fa_sparse``.
"""
from __future__ import annotations

from typing import NamedTuple

import torch
import torch.nn as nn
from torch import distributions


def _dist(cls, *args, **kwargs):
    """A torch distribution whose argument validation (one host sync per constrained argument) moves to the end of an
    enclosing ``ops.deferred_info()`` block -- the training loops' steps; the plain constructor elsewhere."""
    from .ops import checked_dist
    return checked_dist(cls, *args, **kwargs)


class GaussianLikelihood(nn.Module):
    """pY = Normal(F, softplus(noise)) with F ~ qF.rsample((E,)); reference likelihoods.py:7-20."""

    def __init__(self, gp, noise=0.1):
        super().__init__()
        self.gp = gp
        self.noise = nn.Parameter(torch.tensor(noise))

    def forward(self, X, E=1, verbose=False, **kwargs):
        qF, qU, pU = self.gp(X, verbose=verbose, **kwargs)
        F = qF.rsample((E,))
        pY = _dist(distributions.Normal, F, torch.nn.functional.softplus(self.noise))
        return pY, qF, qU, pU


class ExactLikelihood(nn.Module):
    """pY = Normal(qF.mean, softplus(noise)); reference likelihoods.py:23-36.  ``elbo`` evaluates
    the closed-form objective of mggp_test_exact.ipynb:157-159 in the same fused pass."""

    def __init__(self, gp, noise=0.1):
        super().__init__()
        self.gp = gp
        self.noise = nn.Parameter(torch.tensor(noise))

    def forward(self, X, E=1, verbose=False, **kwargs):
        qF, qU, pU = self.gp(X, verbose=verbose, **kwargs)
        pY = _dist(distributions.Normal, qF.mean, torch.nn.functional.softplus(self.noise))
        return pY, qF, qU, pU

    def elbo(self, X, y, **kwargs):
        sd = float(torch.nn.functional.softplus(self.noise.detach()))
        return self.gp.elbo(X, y, sd, groupsX=kwargs.get('groupsX'))[0]


# --------------------------------------------------------------------------------------------
# Poisson factor models (SURVEY.md §8f "next" #2).  The classes keep the reference's names,
# constructor signatures, parameter names and return tuples (pY is a real torch Poisson over the
# (E,D,N) rate, because callers use pY.log_prob / pY.rate); `expected_loglik` is the fused
# MI355X path for the training step: same number as pY.log_prob(y).mean(0).sum(), same gradients,
# without materialising the rate.
# --------------------------------------------------------------------------------------------

class _PoissonLogLik(torch.autograd.Function):
    """(1/E) sum_e sum_dn log Poisson(y | V Z_e) through gpz_poisson_nsf (forward and gradients in
    one fused pass; backward only scales them)."""

    @staticmethod
    def forward(ctx, mean, scale, W_pos, V_pos, eps, y, with_lgamma):
        from . import ops
        ll, dmean, dscale, dW, dV = ops.poisson_nsf(mean, scale, eps, W_pos, V_pos, y, with_lgamma)
        ctx.save_for_backward(dmean.to(mean.dtype), dscale.to(scale.dtype), dW.to(W_pos.dtype), dV.to(V_pos.dtype))
        return ll.to(mean.dtype)

    @staticmethod
    def backward(ctx, g):
        dmean, dscale, dW, dV = ctx.saved_tensors
        return g * dmean, g * dscale, g * dW, g * dV, None, None, None


class SparseCounts:
    """A (D genes, N spots) count matrix held as its non-zeros, in the two orders gpz_poisson_nsf_sparse reads: by spot
    (``col_ptr`` int64 (N+1), ``col_gene`` int32, ``col_val`` fp32) and by gene (``row_ptr`` int64 (D+1), ``row_spot`` int32,
    ``row_perm`` int32 = position of the same non-zero in the by-spot order).  Built once with torch sorts (stable, so the
    order is fixed); explicit zeros are dropped and duplicate entries summed.

    ``y`` may be a dense (D, N) tensor, a torch sparse tensor (COO, CSR or CSC layout), or any object with ``indptr``,
    ``indices``, ``data``, ``shape`` and ``format in ('csr', 'csc')`` -- what ``adata.X`` is (scipy is not imported).

    ``y[:, idx]`` with a 1-D integer tensor of DISTINCT spots is a light view (this object + ``idx`` + its inverse ``pos``):
    no counts are copied.  It is the expression the mini-batch training loops evaluate, so they, ``train`` and
    ``train_hybrid`` take a ``SparseCounts`` where they take a dense ``y`` (``fused=True``, the default).  Spots out of
    range or listed twice raise IndexError: at the end of an enclosing ``ops.deferred_info()`` block (the training loops'
    steps; the kernel meanwhile reads clamped indices, never out of bounds), otherwise at once, which reads one flag from
    the device.  Any other index form raises TypeError."""

    def __init__(self, y):
        self.base, self.idx, self.pos = self, None, None
        gene, spot, val, (D, N) = _coo_triplets(y)
        D, N = int(D), int(N)
        if D < 1 or N < 1:
            raise ValueError(f"SparseCounts: a (genes, spots) matrix expected, got shape {(D, N)}")
        gene, spot = gene.to(torch.int64).reshape(-1), spot.to(torch.int64).reshape(-1)
        val = val.reshape(-1)
        if gene.numel() != spot.numel() or gene.numel() != val.numel():
            raise ValueError("SparseCounts: index and value arrays of different lengths")
        if gene.numel() and (int(gene.min()) < 0 or int(gene.max()) >= D or int(spot.min()) < 0 or int(spot.max()) >= N):
            raise IndexError(f"SparseCounts: an index lies outside the shape {(D, N)}")
        # by spot, genes ascending inside a spot; duplicates (equal keys, adjacent after the sort) are summed in fp64 in
        # their stored order, then zeros are dropped
        key, order = torch.sort(spot * D + gene, stable=True)
        v = val[order].to(torch.float64)
        if key.numel():
            last = torch.ones_like(key, dtype=torch.bool)
            last[:-1] = key[1:] != key[:-1]
            csum = torch.cumsum(v, 0)[last]
            v = torch.diff(csum, prepend=csum.new_zeros(1))
            key = key[last]
        keep = v != 0
        key, v = key[keep], v[keep]
        spot, gene = torch.div(key, D, rounding_mode="floor"), key % D
        if key.numel() >= 2 ** 31:
            raise ValueError("SparseCounts: 2^31 or more non-zeros")
        self.shape = (D, N)
        self.col_val = v.to(torch.float32).contiguous()
        self.col_gene = gene.to(torch.int32).contiguous()
        self.col_ptr = _offsets(spot, N)
        perm = torch.sort(gene, stable=True).indices          # by gene, spots ascending inside a gene
        self.row_perm = perm.to(torch.int32).contiguous()
        self.row_spot = spot[perm].to(torch.int32).contiguous()
        self.row_ptr = _offsets(gene, D)

    _PARTS = ("col_ptr", "col_gene", "col_val", "row_ptr", "row_spot", "row_perm")

    @property
    def device(self):
        return self.base.col_val.device

    @property
    def nnz(self) -> int:
        """Stored non-zeros; of a view, those of its spots (read from the device)."""
        if self.base is self:
            return int(self.col_val.numel())
        cp = self.base.col_ptr
        return int((cp[self.idx.long() + 1] - cp[self.idx.long()]).sum())

    def to(self, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self.device:
            return self
        out = object.__new__(SparseCounts)
        if self.base is self:
            out.base, out.idx, out.pos, out.shape = out, None, None, self.shape
            for k in self._PARTS:
                setattr(out, k, getattr(self, k).to(device))
        else:
            out.base, out.idx, out.pos, out.shape = self.base.to(device), self.idx.to(device), self.pos.to(device), self.shape
        return out

    def cuda(self, device=None):
        return self.to(torch.device("cuda") if device is None else device)

    def cpu(self):
        return self.to("cpu")

    def _spots(self):
        """The spot of every stored value, in the by-spot order."""
        b = self.base
        return torch.repeat_interleave(torch.arange(b.shape[1], device=self.device), torch.diff(b.col_ptr))

    def to_dense(self):
        b = self.base
        out = torch.zeros(self.shape, dtype=torch.float32, device=self.device)
        gene, col, val = b.col_gene.long(), b._spots(), b.col_val
        if b is not self:
            col = self.pos.long()[col]
            inside = col >= 0
            gene, col, val = gene[inside], col[inside], val[inside]
        out[gene, col] = val
        return out

    def __getitem__(self, key):
        if not (isinstance(key, tuple) and len(key) == 2 and isinstance(key[0], slice) and key[0] == slice(None)
                and isinstance(key[1], torch.Tensor) and key[1].dim() == 1
                and key[1].dtype in (torch.int32, torch.int64)):
            raise TypeError("SparseCounts supports y[:, idx] with a 1-D integer tensor of distinct spots only "
                            "(y.to_dense() gives the array)")
        if self.base is not self:
            raise TypeError("SparseCounts: y[:, idx] of a view; index the SparseCounts itself")
        N = self.shape[1]
        want = key[1].to(device=self.device, dtype=torch.int64)
        B = int(want.numel())
        if B < 1 or B > N:
            raise IndexError(f"SparseCounts: {B} distinct spots out of {N}")
        want = torch.where(want < 0, want + N, want)              # negative indices count from the end, as for a tensor
        idx = want.clamp(0, N - 1)
        ar = torch.arange(B, dtype=torch.int32, device=self.device)
        pos = torch.full((N,), -1, dtype=torch.int32, device=self.device)
        pos[idx] = ar
        ok = (idx == want).all() & (pos[idx] == ar).all()

        def fail():
            raise IndexError(f"SparseCounts: y[:, idx] needs distinct spots in [0, {N}): an index is out of range or repeated")
        from .ops import _deferring
        d = _deferring()
        if d is not None:
            d.add_flag(ok, fail)
        elif not bool(ok):
            fail()
        out = object.__new__(SparseCounts)
        out.base, out.idx, out.pos, out.shape = self, idx.to(torch.int32), pos, (self.shape[0], B)
        return out

    def select_genes(self, genes):
        """A whole ``SparseCounts`` of the rows ``genes`` in that order -- ``SparseCounts(y.to_dense()[genes])`` without the
        dense array: the reference's ``ad[:, :nfeat]`` once ``genes`` is a ranking (``utilities.rank_genes``).  ``genes``: a
        1-D int32 / int64 tensor, or a sequence, of distinct genes in [0, D); a repeated or out-of-range gene raises
        IndexError.  Torch ops on this object's device, one pass over the stored entries and the constructor's two sorts;
        the values are carried over as they are.  Of a view ``y[:, idx]``: TypeError."""
        if self.base is not self:
            raise TypeError("SparseCounts: select_genes of a view y[:, idx]; select from the SparseCounts itself")
        D, N = self.shape
        dev = self.device
        g = _gene_index(genes, D, dev, "SparseCounts.select_genes")
        G = int(g.numel())
        new_id = torch.full((D,), -1, dtype=torch.int64, device=dev)
        new_id[g] = torch.arange(G, dtype=torch.int64, device=dev)
        gene = new_id[self.col_gene.long()]
        keep = gene >= 0
        gene, spot, val = gene[keep], self._spots()[keep], self.col_val[keep]
        order = torch.sort(spot * G + gene, stable=True).indices      # by spot, the new ids ascending inside a spot
        gene, spot = gene[order], spot[order]
        out = object.__new__(SparseCounts)
        out.base, out.idx, out.pos, out.shape = out, None, None, (G, N)
        out.col_val = val[order].contiguous()
        out.col_gene = gene.to(torch.int32).contiguous()
        out.col_ptr = _offsets(spot, N)
        perm = torch.sort(gene, stable=True).indices
        out.row_perm = perm.to(torch.int32).contiguous()
        out.row_spot = spot[perm].to(torch.int32).contiguous()
        out.row_ptr = _offsets(gene, G)
        return out

    @property
    def T(self):
        """The (N spots, D genes) orientation of the same counts, a ``TransposedCounts``: what ``regularized_nmf`` and
        ``scanpy_sizefactors`` take (obs x feat).  Nothing is copied.  Of a view ``y[:, idx]``: TypeError (the
        factorisation is of the whole data set)."""
        if self.base is not self:
            raise TypeError("SparseCounts: .T of a view y[:, idx]; the NMF start is computed from the whole data set "
                            "(take .T of the SparseCounts itself)")
        return TransposedCounts(self)

    def __repr__(self):
        return f"SparseCounts(shape={tuple(self.shape)}, device={self.device}{'' if self.base is self else ', view'})"


class TransposedCounts:
    """``counts.T``: a ``SparseCounts`` (D genes, N spots) read as the (N, D) obs x feat matrix X[n, d] = counts[d, n].
    Holds the counts object and the dtype (``torch.float32`` unless ``.double()``) a factorisation of it runs in; no
    counts are copied.  ``.T`` gives the counts back."""

    def __init__(self, counts, dtype=torch.float32):
        if not isinstance(counts, SparseCounts) or counts.base is not counts:
            raise TypeError("TransposedCounts: a whole SparseCounts expected (counts.T)")
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"TransposedCounts: dtype {dtype} unsupported (torch.float32, torch.float64)")
        self.counts, self.dtype = counts, dtype

    @property
    def T(self):
        return self.counts

    @property
    def shape(self):
        return (self.counts.shape[1], self.counts.shape[0])

    @property
    def device(self):
        return self.counts.device

    @property
    def nnz(self) -> int:
        return self.counts.nnz

    def to(self, device):
        moved = self.counts.to(device)
        return self if moved is self.counts else TransposedCounts(moved, self.dtype)

    def cuda(self, device=None):
        return self.to(torch.device("cuda") if device is None else device)

    def cpu(self):
        return self.to("cpu")

    def double(self):
        return self if self.dtype == torch.float64 else TransposedCounts(self.counts, torch.float64)

    def float(self):
        return self if self.dtype == torch.float32 else TransposedCounts(self.counts, torch.float32)

    def to_dense(self):
        return self.counts.to_dense().T.contiguous()

    def __repr__(self):
        return f"TransposedCounts(shape={self.shape}, dtype={self.dtype}, device={self.device})"


class SparseExpression:
    """The (D genes, N spots) real matrix ``values - offset[:, None]`` held as the stored entries of ``values`` (a
    ``SparseCounts``-structured object: the same six index / value arrays, so the by-spot and by-gene orders are reused)
    and a (D,) fp64 ``offset``.  Centred log-normalised counts are of this form (``utilities.log_normalize``): the values
    have exactly the sparsity of the counts, and nothing of D x N elements is held.

    It is what the Gaussian factor models (``RSF``, ``FA``) take in place of a dense array: ``expected_loglik``, ``score``
    and the training loops evaluate it through gpz_gaussian_fa_sparse.  ``y[:, idx]`` with a 1-D integer tensor of distinct
    spots is a no-copy view (``SparseCounts.__getitem__``, its deferred check included); a view of a view raises TypeError.
    It holds no counts: the Poisson / NB steps, the deviances, ``regularized_nmf`` and ``scanpy_sizefactors`` refuse it."""

    def __init__(self, values, offset):
        if not isinstance(values, SparseCounts):
            raise TypeError(f"SparseExpression: values must be a SparseCounts-structured object, got {type(values).__name__}")
        offset = torch.as_tensor(offset).detach().to(device=values.device, dtype=torch.float64).reshape(-1).contiguous()
        if offset.numel() != values.shape[0]:
            raise ValueError(f"SparseExpression: offset has {offset.numel()} values for {values.shape[0]} genes")
        self.values, self.offset = values, offset

    @property
    def shape(self):
        return self.values.shape

    @property
    def device(self):
        return self.values.device

    @property
    def nnz(self) -> int:
        return self.values.nnz

    @property
    def is_view(self) -> bool:
        return self.values.base is not self.values

    def to(self, device):
        moved = self.values.to(device)
        return self if moved is self.values else SparseExpression(moved, self.offset.to(moved.device))

    def cuda(self, device=None):
        return self.to(torch.device("cuda") if device is None else device)

    def cpu(self):
        return self.to("cpu")

    def to_dense(self):
        """The (D, N) array in fp32 (of a view: its B columns): ``values.to_dense() - offset[:, None]``, formed in fp64."""
        return (self.values.to_dense().double() - self.offset[:, None]).to(torch.float32)

    def __getitem__(self, key):
        if self.is_view:
            raise TypeError("SparseExpression: y[:, idx] of a view; index the SparseExpression itself")
        return SparseExpression(self.values[key], self.offset)

    def select_genes(self, genes):
        """A whole ``SparseExpression`` of the rows ``genes`` in that order (``SparseCounts.select_genes`` of the values,
        ``offset[genes]`` carried along).  Of a view: TypeError."""
        if self.is_view:
            raise TypeError("SparseExpression: select_genes of a view y[:, idx]; select from the SparseExpression itself")
        g = _gene_index(genes, self.shape[0], self.device, "SparseExpression.select_genes")
        return SparseExpression(self.values.select_genes(g), self.offset[g])

    def __repr__(self):
        return f"SparseExpression(shape={tuple(self.shape)}, device={self.device}{', view' if self.is_view else ''})"


def _counts_expected(y, who):
    """A ``SparseExpression`` holds real-valued expression, not counts: the count likelihoods refuse it."""
    if isinstance(y, SparseExpression):
        raise TypeError(f"{who}: a SparseExpression holds real-valued expression (values - offset), not counts; the count "
                        "likelihoods take a SparseCounts or a dense count array, the Gaussian models (RSF, FA) take this")


def _gene_index(genes, D, device, who):
    """``genes`` as a 1-D int64 tensor on ``device``: distinct values in [0, D), or IndexError."""
    if isinstance(genes, (SparseCounts, SparseExpression, TransposedCounts, str)):
        raise TypeError(f"{who}: genes must be a 1-D integer tensor or a sequence of gene indices, got {type(genes).__name__}")
    g = genes.detach() if isinstance(genes, torch.Tensor) else torch.as_tensor(genes)
    if g.numel() == 0:
        raise IndexError(f"{who}: no gene selected")
    if g.dtype not in (torch.int32, torch.int64):
        if g.is_floating_point() or g.is_complex() or g.dtype == torch.bool:
            raise TypeError(f"{who}: genes must hold integer indices, got {g.dtype}")
        g = g.to(torch.int64)
    if g.dim() != 1:
        raise ValueError(f"{who}: genes must be 1-D, got shape {tuple(g.shape)}")
    g = g.to(device=device, dtype=torch.int64)
    if g.numel() < 1 or g.numel() > D:
        raise IndexError(f"{who}: {g.numel()} distinct genes out of {D}")
    seen = torch.zeros(D, dtype=torch.int64, device=device)
    inside = (g >= 0) & (g < D)
    seen.scatter_add_(0, g.clamp(0, D - 1), torch.ones_like(g))
    if not bool(inside.all() & (seen <= 1).all()):
        raise IndexError(f"{who}: distinct genes in [0, {D}) needed: an index is out of range or repeated")
    return g


def _segment_sums(v, ptr):
    """fp64 sums of the runs ``v[ptr[i]:ptr[i + 1]]`` in a fixed order (0 for an empty run)."""
    v = v.to(torch.float64)
    if v.numel() == 0:
        return torch.zeros(ptr.numel() - 1, dtype=torch.float64, device=ptr.device)
    return torch.segment_reduce(v, "sum", lengths=torch.diff(ptr), unsafe=True)


def _gene_moments(expr):
    """(sum_n z, sum_n z^2) per gene over all spots of a whole ``SparseExpression``, fp64."""
    v = expr.values
    z = v.col_val[v.row_perm.long()].to(torch.float64)
    return _segment_sums(z, v.row_ptr), _segment_sums(z * z, v.row_ptr)


def _offsets(sorted_ids, n):
    """(n + 1,) int64 start offsets of the runs of an ascending id array."""
    out = torch.zeros(n + 1, dtype=torch.int64, device=sorted_ids.device)
    if sorted_ids.numel():
        out[1:] = torch.cumsum(torch.bincount(sorted_ids, minlength=n), 0)
    return out


def _expand_ptr(ptr, n):
    ptr = ptr.to(torch.int64)
    return torch.repeat_interleave(torch.arange(n, device=ptr.device), torch.diff(ptr))


def _coo_triplets(y):
    """(gene, spot, value, shape) of whatever SparseCounts accepts; duplicates and zeros still in."""
    if isinstance(y, SparseCounts):
        b = y.base
        if b is not y:
            raise TypeError("SparseCounts: built from a view; use y.to_dense() or the parent")
        return b.col_gene, b._spots(), b.col_val, b.shape
    if isinstance(y, torch.Tensor):
        y = y.detach()
        if y.dim() != 2:
            raise ValueError(f"SparseCounts: a (genes, spots) matrix expected, got {y.dim()} dimensions")
        if y.layout == torch.strided:
            gene, spot = torch.nonzero(y, as_tuple=True)
            return gene, spot, y[gene, spot], y.shape
        if y.layout == torch.sparse_coo:
            ind = y._indices()
            return ind[0], ind[1], y._values(), y.shape
        if y.layout == torch.sparse_csr:
            return _expand_ptr(y.crow_indices(), y.shape[0]), y.col_indices(), y.values(), y.shape
        if y.layout == torch.sparse_csc:
            return y.row_indices(), _expand_ptr(y.ccol_indices(), y.shape[1]), y.values(), y.shape
        raise TypeError(f"SparseCounts: tensor layout {y.layout} unsupported (strided, COO, CSR, CSC)")
    fmt = getattr(y, "format", None)
    if fmt in ("csr", "csc") and all(hasattr(y, k) for k in ("indptr", "indices", "data", "shape")):
        indptr, indices, data = (torch.as_tensor(getattr(y, k)) for k in ("indptr", "indices", "data"))
        D, N = y.shape
        if indptr.numel() != (D if fmt == "csr" else N) + 1:
            raise ValueError(f"SparseCounts: indptr of {indptr.numel()} entries for a {fmt} matrix of shape {(D, N)}")
        major = _expand_ptr(indptr, D if fmt == "csr" else N)
        return (major, indices, data, (D, N)) if fmt == "csr" else (indices, major, data, (D, N))
    raise TypeError(f"SparseCounts: cannot read counts from {type(y).__name__} (a dense or sparse torch tensor, or an "
                    "object with indptr, indices, data, shape and format 'csr' / 'csc')")


class _SparsePoissonLogLik(torch.autograd.Function):
    """_PoissonLogLik for a SparseCounts (or its view y[:, idx]) through gpz_poisson_nsf_sparse."""

    @staticmethod
    def forward(ctx, mean, scale, W_pos, V_pos, eps, y, with_lgamma):
        from . import ops
        ll, dmean, dscale, dW, dV = ops.poisson_nsf_sparse(mean, scale, eps, W_pos, V_pos, y, None, with_lgamma)
        ctx.save_for_backward(dmean.to(mean.dtype), dscale.to(scale.dtype), dW.to(W_pos.dtype), dV.to(V_pos.dtype))
        return ll.to(mean.dtype)

    @staticmethod
    def backward(ctx, g):
        dmean, dscale, dW, dV = ctx.saved_tensors
        return g * dmean, g * dscale, g * dW, g * dV, None, None, None


def _loglik_function(y):
    """The autograd function of the fused Poisson step for this form of the counts: the caller chooses by what they pass."""
    _counts_expected(y, "poisson_expected_loglik")
    return _SparsePoissonLogLik if isinstance(y, SparseCounts) else _PoissonLogLik


def poisson_expected_loglik(qF_list, W_list, V_pos, y, E=10, with_lgamma=True, eps=None):
    """Fused Monte-Carlo E_q[log p(y | F)] for rate = V * sum_k W_k exp(F_k), F_k ~ qF_k.

    qF_list: Normal distributions over (L_k, N) factors; W_list: positive (D, L_k) loadings; y: the (D, N) counts, dense
    (gpz_poisson_nsf) or a ``SparseCounts`` / its view ``y[:, idx]`` (gpz_poisson_nsf_sparse)."""
    mean = torch.cat([q.mean for q in qF_list], dim=0)
    scale = torch.cat([q.scale for q in qF_list], dim=0)
    W = torch.cat(list(W_list), dim=1)
    if eps is None:   # one draw per factor set, in order, through the function Normal.rsample itself uses
        import torch.distributions.normal as tdn
        eps = torch.cat([tdn._standard_normal((E,) + tuple(q.mean.shape), dtype=mean.dtype, device=mean.device)
                         for q in qF_list], dim=1)
    return _loglik_function(y).apply(mean, scale, W, V_pos, eps, y, with_lgamma)


class _NBLogLik(torch.autograd.Function):
    """(1/E) sum_e sum_dn log NegativeBinomial(y | total_count = theta_d, mean = V Z_e) through gpz_nb_nsf (forward and
    gradients in one fused pass; backward only scales them)."""

    @staticmethod
    def forward(ctx, mean, scale, W_pos, V_pos, theta_pos, eps, y, with_lgamma):
        from . import ops
        ll, dmean, dscale, dW, dV, dtheta = ops.nb_nsf(mean, scale, eps, W_pos, V_pos, theta_pos, y, with_lgamma)
        ctx.save_for_backward(dmean.to(mean.dtype), dscale.to(scale.dtype), dW.to(W_pos.dtype), dV.to(V_pos.dtype),
                              dtheta.to(theta_pos.dtype))
        return ll.to(mean.dtype)

    @staticmethod
    def backward(ctx, g):
        dmean, dscale, dW, dV, dtheta = ctx.saved_tensors
        return g * dmean, g * dscale, g * dW, g * dV, g * dtheta, None, None, None


class _SparseNBLogLik(torch.autograd.Function):
    """_NBLogLik for a SparseCounts (or its view y[:, idx]) through gpz_nb_nsf_sparse."""

    @staticmethod
    def forward(ctx, mean, scale, W_pos, V_pos, theta_pos, eps, y, with_lgamma):
        from . import ops
        ll, dmean, dscale, dW, dV, dtheta = ops.nb_nsf_sparse(mean, scale, eps, W_pos, V_pos, theta_pos, y, None, with_lgamma)
        ctx.save_for_backward(dmean.to(mean.dtype), dscale.to(scale.dtype), dW.to(W_pos.dtype), dV.to(V_pos.dtype),
                              dtheta.to(theta_pos.dtype))
        return ll.to(mean.dtype)

    @staticmethod
    def backward(ctx, g):
        dmean, dscale, dW, dV, dtheta = ctx.saved_tensors
        return g * dmean, g * dscale, g * dW, g * dV, g * dtheta, None, None, None


def _nb_loglik_function(y):
    """The autograd function of the fused negative-binomial step for this form of the counts (``_loglik_function``'s sibling)."""
    _counts_expected(y, "nb_expected_loglik")
    return _SparseNBLogLik if isinstance(y, SparseCounts) else _NBLogLik


def nb_expected_loglik(qF_list, W_list, V_pos, theta_pos, y, E=10, with_lgamma=True, eps=None):
    """``poisson_expected_loglik`` under pY = NegativeBinomial(total_count=theta[:, None], logits=log(rate) - log(theta[:, None])),
    rate = V * sum_k W_k exp(F_k): theta_pos (D,) positive inverse dispersions, variance rate + rate^2 / theta.  ``eps`` is
    drawn exactly as there.  y: the (D, N) counts, dense (gpz_nb_nsf) or a ``SparseCounts`` / its view ``y[:, idx]``
    (gpz_nb_nsf_sparse: the zero-count term -theta log1p(rate / theta) is a dense pass that reads no counts, the rest a sum
    over the non-zeros)."""
    mean = torch.cat([q.mean for q in qF_list], dim=0)
    scale = torch.cat([q.scale for q in qF_list], dim=0)
    W = torch.cat(list(W_list), dim=1)
    if eps is None:   # one draw per factor set, in order, through the function Normal.rsample itself uses
        import torch.distributions.normal as tdn
        eps = torch.cat([tdn._standard_normal((E,) + tuple(q.mean.shape), dtype=mean.dtype, device=mean.device)
                         for q in qF_list], dim=1)
    return _nb_loglik_function(y).apply(mean, scale, W, V_pos, theta_pos, eps, y, with_lgamma)


LIKELIHOODS = ("poisson", "nb")


def _init_likelihood(module, likelihood, theta0, D):
    """The ``likelihood=`` / ``theta0=`` keywords of the count models.  "poisson" adds nothing (the parameters stay the
    reference's); "nb" adds ``theta`` (D,), raw, with softplus(theta) = theta0 (``init_softplus``).

    ``theta0``: one positive number for every gene, or a (D,) array or tensor of finite positive values, e.g. the start from
    a gene-wise fit, ``theta0=disp.theta.nan_to_num(nan=10.0).clamp(1e-2, 1e3)`` with ``disp = gene_dispersion(y)``.  That
    fit holds each gene's rate at the constant-rate null, which absorbs the biological variation the factors will explain:
    its theta is a lower-biased start, not an estimate of the model's theta."""
    if likelihood not in LIKELIHOODS:
        raise ValueError(f"{type(module).__name__}: likelihood={likelihood!r} unknown (one of {LIKELIHOODS})")
    module.likelihood = likelihood
    if likelihood == "nb":
        import numpy as np
        from .utilities import init_softplus
        who = type(module).__name__
        if isinstance(theta0, (list, tuple)) or (isinstance(theta0, (torch.Tensor, np.ndarray)) and theta0.ndim > 0):
            start = (theta0.detach().cpu() if isinstance(theta0, torch.Tensor) else torch.as_tensor(np.asarray(theta0))).double().numpy()
            if start.shape != (D,):
                raise ValueError(f"{who}: theta0 of shape {start.shape} for {D} genes (a number or ({D},) values expected)")
            if not (np.isfinite(start).all() and (start > 0).all()):
                raise ValueError(f"{who}: every theta0 must be positive and finite")
        else:
            if not float(theta0) > 0:
                raise ValueError(f"{who}: theta0 must be positive, got {theta0}")
            start = np.full((D,), float(theta0), dtype=np.float64)
        raw = init_softplus(start)
        module.theta = nn.Parameter(torch.as_tensor(raw, dtype=torch.get_default_dtype()))


def _count_dist(module, rate):
    """pY of a count model over its rate: Poisson, or the negative binomial with the model's per-gene theta."""
    if getattr(module, "likelihood", "poisson") == "nb":
        th = torch.nn.functional.softplus(module.theta)[:, None]
        return _dist(distributions.NegativeBinomial, total_count=th, logits=torch.log(rate) - torch.log(th))
    return _dist(distributions.Poisson, rate)


def _expected_loglik(module, qF_list, W_list, V_pos, y, E, with_lgamma, eps):
    """The fused training-step value of a count model under its likelihood."""
    if getattr(module, "likelihood", "poisson") == "nb":
        return nb_expected_loglik(qF_list, W_list, V_pos, torch.nn.functional.softplus(module.theta), y, E=E,
                                  with_lgamma=with_lgamma, eps=eps)
    return poisson_expected_loglik(qF_list, W_list, V_pos, y, E=E, with_lgamma=with_lgamma, eps=eps)


class PoissonDeviance(NamedTuple):
    """What ``poisson_deviance`` returns; every tensor is fp64 and carries no graph.  ``mean`` = total / (D B);
    ``explained`` = 1 - total / null_total and ``explained_per_gene`` likewise (NaN where the null deviance is 0);
    ``sum_mu / sum_y`` is the calibration of the size factors."""
    total: torch.Tensor
    mean: torch.Tensor
    per_gene: torch.Tensor
    per_spot: torch.Tensor
    null_total: torch.Tensor
    null_per_gene: torch.Tensor
    explained: torch.Tensor
    explained_per_gene: torch.Tensor
    sum_y: torch.Tensor
    sum_mu: torch.Tensor


def _explained(dev, null):
    return torch.where(null == 0, torch.full_like(null, float("nan")), 1.0 - dev / torch.where(null == 0, torch.ones_like(null), null))


def poisson_deviance(qF_list, W_list, V_pos, y, *, lognormal_mean=True):
    """Poisson deviance of the counts ``y`` under the predictive mean rate mu = V * sum_k W_k E_q[exp F_k], exactly (no
    sampling): E_q[exp F] = exp(mean + scale^2 / 2), or the plug-in exp(mean) with ``lognormal_mean=False``.  The unit
    deviance is 2 (y log(y / mu) - y + mu), 2 mu where y = 0; the null model is one constant rate per gene given V.

    qF_list: Normal distributions over (L_k, B) factors at the B spots being scored; W_list: positive (D, L_k) loadings;
    V_pos (B,) positive size factors; y: the (D, B) counts, dense (gpz_poisson_deviance) or a ``SparseCounts`` / its view
    ``y[:, idx]`` (gpz_poisson_deviance_sparse).  The (D, B) rate is never materialised.  Returns a ``PoissonDeviance``."""
    from . import ops
    _counts_expected(y, "poisson_deviance")
    with torch.no_grad():
        mean = torch.cat([q.mean for q in qF_list], dim=0)
        scale = torch.cat([q.scale for q in qF_list], dim=0)
        W = torch.cat(list(W_list), dim=1)
        if isinstance(y, SparseCounts):
            r = ops.poisson_deviance_sparse(mean, scale, W, V_pos, y, None, lognormal_mean)
        else:
            r = ops.poisson_deviance(mean, scale, W, V_pos, y, lognormal_mean)
        D, B = y.shape
        return PoissonDeviance(total=r["total"], mean=r["total"] / (D * B), per_gene=r["per_gene"], per_spot=r["per_spot"],
                               null_total=r["null_total"], null_per_gene=r["null_per_gene"],
                               explained=_explained(r["total"], r["null_total"]),
                               explained_per_gene=_explained(r["per_gene"], r["null_per_gene"]),
                               sum_y=r["sum_y"], sum_mu=r["sum_mu"])


class NBDeviance(NamedTuple):
    """What ``nb_deviance`` returns; every tensor is fp64 and carries no graph.  The first ten fields have the names and
    meanings of ``PoissonDeviance``, for the negative-binomial unit deviance with the per-gene ``theta``.  ``loglik`` is the
    NB log density of the counts, ``poisson_loglik`` the Poisson log density under the same rate: ``loglik -
    poisson_loglik`` (in total, or ``loglik_per_gene - poisson_loglik_per_gene``) is what the dispersion parameter earned,
    in comparable units -- deviances of different families are not comparable."""
    total: torch.Tensor
    mean: torch.Tensor
    per_gene: torch.Tensor
    per_spot: torch.Tensor
    null_total: torch.Tensor
    null_per_gene: torch.Tensor
    explained: torch.Tensor
    explained_per_gene: torch.Tensor
    sum_y: torch.Tensor
    sum_mu: torch.Tensor
    loglik: torch.Tensor
    loglik_per_gene: torch.Tensor
    loglik_per_spot: torch.Tensor
    poisson_loglik: torch.Tensor
    poisson_loglik_per_gene: torch.Tensor
    theta: torch.Tensor


def nb_deviance(qF_list, W_list, V_pos, theta_pos, y, *, lognormal_mean=True):
    """Negative-binomial scoring of the counts ``y`` under the predictive mean rate of ``poisson_deviance`` and one inverse
    dispersion ``theta_pos`` (D,) > 0 per gene (variance mu + mu^2 / theta): the unit deviance
    2 [y log(y / mu) - (y + theta) log1p((y - mu) / (mu + theta))], the log density log NB(y | mu, theta) and the Poisson log
    density of the same mu, per gene, per spot and in total.

    The null model is one constant rate per gene given V, r_d = sum_n y / sum_n V, with the gene's own theta.  That rate is
    the null's maximum-likelihood rate when V is constant; otherwise it is a convention, the one ``PoissonDeviance`` uses.

    Arguments as for ``poisson_deviance``; y dense (gpz_nb_deviance) or a ``SparseCounts`` / its view ``y[:, idx]``
    (gpz_nb_deviance_sparse).  Returns an ``NBDeviance``."""
    from . import ops
    _counts_expected(y, "nb_deviance")
    with torch.no_grad():
        mean = torch.cat([q.mean for q in qF_list], dim=0)
        scale = torch.cat([q.scale for q in qF_list], dim=0)
        W = torch.cat(list(W_list), dim=1)
        if isinstance(y, SparseCounts):
            r = ops.nb_deviance_sparse(mean, scale, W, V_pos, theta_pos, y, None, lognormal_mean)
        else:
            r = ops.nb_deviance(mean, scale, W, V_pos, theta_pos, y, lognormal_mean)
        D, B = y.shape
        return NBDeviance(total=r["total"], mean=r["total"] / (D * B), per_gene=r["per_gene"], per_spot=r["per_spot"],
                          null_total=r["null_total"], null_per_gene=r["null_per_gene"],
                          explained=_explained(r["total"], r["null_total"]),
                          explained_per_gene=_explained(r["per_gene"], r["null_per_gene"]),
                          sum_y=r["sum_y"], sum_mu=r["sum_mu"], loglik=r["loglik"], loglik_per_gene=r["loglik_per_gene"],
                          loglik_per_spot=r["loglik_per_spot"], poisson_loglik=r["poisson_loglik"],
                          poisson_loglik_per_gene=r["poisson_loglik_per_gene"],
                          theta=theta_pos.detach().to(torch.float32).double())


def _deviance_theta(module, raw_W, family, theta):
    """The per-gene theta ``deviance`` scores with, or None for the Poisson deviance.  ``family``: "poisson", "nb", or
    "model" (the model's own likelihood).  ``theta``: positive, a scalar or (D,), in place of softplus(module.theta) --
    it scores a Poisson-fitted model under a chosen dispersion (a tensor on the device is not checked for its sign: that
    would wait for the device)."""
    who = type(module).__name__
    if family == "model":
        family = getattr(module, "likelihood", "poisson")
    if family not in ("poisson", "nb"):
        raise ValueError(f'{who}.deviance: family must be "poisson", "nb" or "model", got {family!r}')
    if family == "poisson":
        if theta is not None:
            raise ValueError(f'{who}.deviance: theta= belongs to family="nb"')
        return None
    D = raw_W.shape[0]
    if theta is None:
        raw = getattr(module, "theta", None)
        if raw is None:
            raise ValueError(f'{who}.deviance: family="nb" on a model without theta (likelihood="poisson") needs theta=')
        return torch.nn.functional.softplus(raw.detach())
    th = torch.as_tensor(theta, dtype=torch.float32) if not isinstance(theta, torch.Tensor) else theta.detach()
    if th.numel() not in (1, D):
        raise ValueError(f"{who}.deviance: theta has {th.numel()} values for {D} genes (a scalar or one per gene)")
    if not th.is_cuda and not bool((th > 0).all()):
        raise ValueError(f"{who}.deviance: theta must be positive")
    return th.to(device=raw_W.device, dtype=torch.float32).reshape(-1).expand(D).contiguous()


def _deviance_of(qF_list, W_list, Vp, theta_pos, y, lognormal_mean):
    if theta_pos is None:
        return poisson_deviance(qF_list, W_list, Vp, y, lognormal_mean=lognormal_mean)
    return nb_deviance(qF_list, W_list, Vp, theta_pos, y, lognormal_mean=lognormal_mean)


def _deviance_size_factors(raw_V, idx, V, n_spots, who):
    """The positive size factors of ``deviance``: the caller's ``V`` or softplus of the model's (indexed by ``idx``)."""
    if V is None:
        V = torch.nn.functional.softplus(raw_V)
        V = V if idx is None else V[idx]
    V = torch.as_tensor(V).reshape(-1)
    if V.numel() != n_spots:
        raise ValueError(f"{who}.deviance: {V.numel()} size factors for {n_spots} spots"
                         + ("" if idx is not None else " (held-out spots need explicit positive size factors V=)"))
    return V


def _hybrid_spots(n_fitted, n_spots, idx, V, who):
    """The hybrids' non-spatial factors exist only for the fitted spots."""
    if idx is None and n_spots != n_fitted:
        raise ValueError(f"{who}.deviance: the non-spatial factors exist only for the {n_fitted} fitted spots, so {n_spots} "
                         "other spots cannot be scored" + (" (V= does not change that)" if V is not None else ""))


class ResidualAutocorr(NamedTuple):
    """What ``residual_autocorr`` returns; every tensor is fp64 and carries no graph.  ``I`` (D,): Moran's I of each gene's
    residuals over the spots' neighbour graph.  ``expected`` and ``variance``: 0-d, the moments of I under normality for that
    graph (they depend on the graph alone).  ``z`` = (I - expected) / sqrt(variance) (D,).  ``residual_mean`` and
    ``residual_var`` (D,): each gene's residual mean and variance over the spots -- near 0 and 1 for Pearson residuals of a
    well-calibrated fit."""
    I: torch.Tensor
    expected: torch.Tensor
    variance: torch.Tensor
    z: torch.Tensor
    residual_mean: torch.Tensor
    residual_var: torch.Tensor


class ResidualGeary(NamedTuple):
    """``residual_autocorr(mode="geary")``: Geary's C of each gene's residuals, fp64 tensors: ``C`` (D,), ``expected`` = 1,
    ``variance`` (0-d under normality, (D,) under randomisation), ``z`` = (C - 1) / sqrt(variance) (D,) -- C < 1, a NEGATIVE
    z, is positive autocorrelation -- and the residuals' ``residual_mean``, ``residual_var`` and ``residual_kurtosis``
    (m4 / m2^2; 3 for a normal sample) (D,)."""
    C: torch.Tensor
    expected: torch.Tensor
    variance: torch.Tensor
    z: torch.Tensor
    residual_mean: torch.Tensor
    residual_var: torch.Tensor
    residual_kurtosis: torch.Tensor


class ResidualAutocorrPerm(NamedTuple):
    """``residual_autocorr(n_perms=)``: the fields of ``ResidualAutocorr``, ``residual_kurtosis``, and the permutation
    null's fields with the meaning they have in ``utilities.GeneAutocorrPerm``: ``n_perms`` = P; ``n_ge`` / ``n_le`` the
    permutations whose I is >= / <= the observed one; ``pval_greater`` = (n_ge + 1) / (P + 1), the p-value for positive
    autocorrelation; ``pval_less``; ``pval_sim`` the smaller of the two; ``mean_sim``, ``var_sim``, ``z_sim``,
    ``pval_z_sim`` of the simulated I; ``sims`` (D, P) or None."""
    I: torch.Tensor
    expected: torch.Tensor
    variance: torch.Tensor
    z: torch.Tensor
    residual_mean: torch.Tensor
    residual_var: torch.Tensor
    residual_kurtosis: torch.Tensor
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
    sims: "torch.Tensor | None"


class ResidualGearyPerm(NamedTuple):
    """``residual_autocorr(mode="geary", n_perms=)``: the fields of ``ResidualGeary`` and the permutation null's, as in
    ``ResidualAutocorrPerm`` with C for I -- so ``pval_less`` = (n_le + 1) / (P + 1) is the p-value for positive
    autocorrelation (a small C) and ``pval_greater`` the one for negative."""
    C: torch.Tensor
    expected: torch.Tensor
    variance: torch.Tensor
    z: torch.Tensor
    residual_mean: torch.Tensor
    residual_var: torch.Tensor
    residual_kurtosis: torch.Tensor
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
    sims: "torch.Tensor | None"


def _cat_factors(qF_list, W_list):
    return (torch.cat([q.mean for q in qF_list], dim=0), torch.cat([q.scale for q in qF_list], dim=0),
            torch.cat(list(W_list), dim=1))


def _residual_null_args(who, B, mode, assumption, n_perms, perms):
    """The refusals of the new keywords that need no device: (permute, P, perms or None)."""
    from .utilities import _autocorr_perms
    if mode not in ("moran", "geary"):
        raise ValueError(f"{who}: mode={mode!r} unknown ('moran', 'geary')")
    if assumption not in ("normality", "randomisation"):
        raise ValueError(f"{who}: assumption={assumption!r} unknown ('normality', 'randomisation')")
    if assumption == "randomisation" and B < 4:
        raise ValueError(f"{who}: assumption='randomisation' needs B >= 4 spots, got {B}")
    if n_perms is None and perms is None:
        return False, 0, None
    return (True, *_autocorr_perms(who, B, n_perms, perms))


def residual_autocorr(qF_list, W_list, V_pos, y, nbr, *, theta_pos=None, kind="pearson", lognormal_mean=True, slab_genes=0,
                      mode="moran", assumption="normality", n_perms=None, seed=0, perms=None, return_sims=False):
    """Is spatial structure left in what the model did not explain, and in which genes: Moran's I of every gene's residuals
    under the predictive mean rate mu = V * sum_k W_k E_q[exp F_k] (as in ``poisson_deviance``) over the neighbour table
    ``nbr`` (B, K) of the B scored spots -- the evidence for adding factors, shortening a length scale or moving a gene to
    the spatial part of a hybrid.  ``kind``: "pearson", (y - mu) / sqrt(mu (1 + mu / theta)), or "deviance",
    sign(y - mu) sqrt(unit deviance); ``theta_pos`` (D,) selects the negative binomial, None the Poisson family.  ``y``: dense
    (D, B) counts or a whole ``SparseCounts``.  Neither the (D, B) rate nor the residuals are materialised
    (``ops.residual_morans_i``).  Returns a ``ResidualAutocorr``.

    ``z`` uses squidpy's normal approximation of I's moments under no autocorrelation and ignores the degrees of freedom
    the fit used: it ranks genes, it is not a calibrated test.

    The keywords below have the meaning they have in ``utilities.gene_autocorr``; with all of them at their defaults the
    call is the one above, bit for bit.  ``mode="geary"`` scores Geary's C (``ops.residual_spatial_stats``) and returns a
    ``ResidualGeary``: 1 in expectation, BELOW 1 -- a negative ``z`` -- for positive autocorrelation.
    ``assumption="randomisation"`` replaces the normality moments, which depend on the graph alone, by the randomisation
    moments of Cliff & Ord at each gene's residual kurtosis (``utilities._autocorr_moments``; B >= 4): ``variance`` and
    ``z`` become (D,) tensors.  Residuals of counts are far from normal -- a single large count gives a gene a kurtosis in
    the hundreds -- so these are the moments to use.  ``n_perms=P`` (permutation p is ``torch.randperm(B, generator=g,
    device=...)`` from one generator seeded with ``seed``, drawn one at a time in order) or ``perms=`` (a (P, B) integer
    tensor, used as given) adds the permutation null, scored while each residual slab is resident
    (``ops.residual_autocorr_perm``), and returns a ``ResidualAutocorrPerm`` / ``ResidualGearyPerm``; ``return_sims=True``
    keeps the (D, P) simulated values.  For Moran ``pval_greater`` is the p-value for positive autocorrelation, for Geary
    ``pval_less``; the smallest attainable value is 1 / (P + 1).  The comparisons are made on the fp64 numerators;
    residuals are real-valued, so a mathematical tie may fall either way in the last bit.

    What the permutation null is and is not: it is exact for exchangeable residuals, and a well-specified fit gives
    approximately exchangeable residuals -- but residuals under a fitted rate are not exactly exchangeable (their variance
    follows the rate, which the Pearson and deviance forms only standardise to first order), and the null still ignores
    the degrees of freedom the fit used, like ``z``.  It calibrates against the residuals' own distribution, which the
    normal approximation does not; it does not turn the score into a test of the model."""
    B = int(nbr.shape[0]) if isinstance(nbr, torch.Tensor) else len(nbr)
    null = _residual_null_args("residual_autocorr", B, mode, assumption, n_perms, perms)
    entries = _count_entries(V_pos, y, nbr, theta_pos, kind, lognormal_mean, slab_genes, mode, return_sims)
    return _residual_autocorr_checked(entries, qF_list, W_list, nbr, null, mode, assumption, seed)


def _count_entries(V_pos, y, nbr, theta_pos, kind, lognormal_mean, slab_genes, mode, return_sims):
    """The count family for ``_residual_autocorr_checked``: (mean, scale, W) -> its Moran-only, wide and permutation entries."""
    from . import ops

    def bind(mean, scale, W):
        head, tail = (mean, scale, W, V_pos, y, nbr), (theta_pos, None, kind, lognormal_mean)
        return (lambda: ops.residual_morans_i(*head, *tail, slab_genes),
                lambda: ops.residual_spatial_stats(*head, *tail, slab_genes),
                lambda perms: ops.residual_autocorr_perm(*head, perms, *tail, stat=mode, return_sims=return_sims,
                                                         slab_genes=slab_genes))
    return bind


def _residual_autocorr_checked(entries, qF_list, W_list, nbr, null, mode, assumption, seed):
    """``residual_autocorr`` and ``gaussian_residual_autocorr`` behind their refusals: ``entries`` is the family
    (``_count_entries``, ``_gaussian_entries``), ``null`` what ``_residual_null_args`` returned for the B scored spots."""
    with torch.no_grad():
        mean, scale, W = _cat_factors(qF_list, W_list)
        return _autocorr_assembly(*entries(mean, scale, W), mean.device, nbr, null, mode, assumption, seed)


def _scored_spot_count(X, idx):
    """The number of scored spots, the rows of ``X[idx]``: ``idx`` None, a boolean mask or a list of indices."""
    if idx is None:
        return int(X.shape[0])
    return int(idx.sum()) if getattr(idx, "dtype", None) == torch.bool else len(idx)


def _autocorr_assembly(narrow, stats, perm, dev, nbr, null, mode, assumption, seed):
    """What the residual entries' outputs become: the moments of the null, z and the permutation fields, as a
    ``ResidualAutocorr`` / ``ResidualGeary`` / ``ResidualAutocorrPerm`` / ``ResidualGearyPerm``.  ``narrow()`` is the
    Moran-only entry (None: the family has none), ``stats()`` the wide entry, ``perm(perms)`` the permutation entry; ``dev`` is
    where the permutations are drawn.  Shared by the count and the Gaussian residuals."""
    from .utilities import _autocorr_moments, _moran_moments, _perm_fields
    permute, P, perms = null
    B = int(nbr.shape[0])
    with torch.no_grad():
        if narrow is not None and mode == "moran" and assumption == "normality" and not permute:
            r = narrow()
            expected, variance = _moran_moments(nbr.to(device=r["I"].device, dtype=torch.int64))
            return ResidualAutocorr(I=r["I"], expected=expected, variance=variance, z=(r["I"] - expected) / torch.sqrt(variance),
                                    residual_mean=r["residual_mean"], residual_var=r["residual_var"])
        if permute:
            if perms is None:
                g = torch.Generator(device=dev)
                g.manual_seed(int(seed))
                perms = torch.empty((P, B), dtype=torch.int32, device=dev)
                for p in range(P):
                    perms[p] = torch.randperm(B, generator=g, device=dev)
            r, mom = perm(perms)
            stat = r.value
        else:
            mom = stats()
            stat = mom["C" if mode == "geary" else "I"]
        table = nbr.to(device=stat.device, dtype=torch.int64)
        if mode == "moran" and assumption == "normality":
            expected, variance = _moran_moments(table)                    # the moments of the call without the new keywords
        else:
            m = _autocorr_moments(table, mom["kurtosis"] if assumption == "randomisation" else None)
            key = ("VC" if mode == "geary" else "VI") + ("_rand" if assumption == "randomisation" else "_norm")
            expected, variance = m["EC" if mode == "geary" else "EI"], m[key]
        base = (stat, expected, variance, (stat - expected) / torch.sqrt(variance), mom["residual_mean"], mom["residual_var"])
        kinds = (ResidualGeary, ResidualGearyPerm) if mode == "geary" else (ResidualAutocorr, ResidualAutocorrPerm)
        if not permute:
            return kinds[0](*base, mom["kurtosis"]) if mode == "geary" else kinds[0](*base)
        return kinds[1](*base, mom["kurtosis"], *_perm_fields(stat, r, P))


def count_residuals(qF_list, W_list, V_pos, y, genes, *, theta_pos=None, kind="pearson", lognormal_mean=True):
    """(len(genes), B) fp32 residuals of the listed genes, gene-major like ``y``, under the rate of ``residual_autocorr``: one
    gene's residual map for plotting.  ``genes``: gene indices in any order, repeats allowed."""
    from . import ops
    if genes is None:
        raise ValueError("count_residuals: genes (a list of gene indices) needed; the full (D, B) array is what this avoids")
    with torch.no_grad():
        mean, scale, W = _cat_factors(qF_list, W_list)
        return ops.count_residuals(mean, scale, W, V_pos, y, theta_pos, genes, kind, lognormal_mean).T.contiguous()


class _ResidualScores:
    """``residual_autocorr`` and ``residuals`` of the count models.  A model supplies ``_score_parts(X, idx, V, kwargs)`` ->
    (qF_list, W_list, V_pos, Xb), the pieces its ``deviance`` assembles."""

    def _residual_theta(self, kind, family, theta):
        """The refusals that need no device, and the per-gene theta (None: Poisson) as ``deviance`` resolves it."""
        if kind not in ("pearson", "deviance"):
            raise ValueError(f'{type(self).__name__}.residual_autocorr: kind must be "pearson" or "deviance", got {kind!r}')
        return _deviance_theta(self, self.sf.W if hasattr(self, "sf") else self.W, family, theta)

    def _residual_data(self, y, what):
        """A refusal of the data's form that a model makes before anything else (``PNMF``); the entries make the rest."""

    def residual_autocorr(self, X, y, idx=None, V=None, *, kind="pearson", family="model", theta=None, n_neighs=6, graph=None,
                          lognormal_mean=True, mode="moran", assumption="normality", n_perms=None, seed=0, perms=None,
                          return_sims=False, **kwargs):
        """Moran's I of every gene's residuals at ``X`` (or ``X[idx]``) over the scored spots' ``n_neighs``-nearest-neighbour
        graph (``ops.spatial_knn``), or over ``graph=``, an (B, K) table: a ``ResidualAutocorr``.  ``y`` (D, B) dense or a
        whole ``SparseCounts``; ``V`` as in ``deviance``.  ``family`` defaults to "model", unlike ``deviance``: residuals are
        standardised by the model's own variance, so an NB fit is scored with its theta (``theta=`` overrides it, or scores
        a Poisson fit under ``family="nb"``).  ``mode``, ``assumption``, ``n_perms``, ``seed``, ``perms`` and
        ``return_sims`` as in ``likelihoods.residual_autocorr``: Geary's C, the randomisation moments and the permutation
        null over the B scored spots; at their defaults the call is the one without them."""
        from . import ops
        self._residual_data(y, "residual_autocorr")
        theta_pos = self._residual_theta(kind, family, theta)
        null = _residual_null_args(f"{type(self).__name__}.residual_autocorr", _scored_spot_count(X, idx), mode, assumption, n_perms,
                                   perms)
        with torch.no_grad():
            qF, W, Vp, Xb = self._score_parts(X, idx, V, kwargs)
            nbr = ops.spatial_knn(Xb, int(n_neighs)) if graph is None else torch.as_tensor(graph)
            entries = _count_entries(Vp, y, nbr, theta_pos, kind, lognormal_mean, 0, mode, return_sims)
            return _residual_autocorr_checked(entries, qF, W, nbr, null, mode, assumption, seed)

    def residuals(self, X, y, genes, idx=None, V=None, *, kind="pearson", family="model", theta=None, lognormal_mean=True,
                  **kwargs):
        """(len(genes), B) fp32 residuals of the listed genes at ``X`` (or ``X[idx]``): the rows ``residual_autocorr`` scores.
        Arguments as there."""
        self._residual_data(y, "residuals")
        theta_pos = self._residual_theta(kind, family, theta)
        with torch.no_grad():
            qF, W, Vp, Xb = self._score_parts(X, idx, V, kwargs)
            return count_residuals(qF, W, Vp, y, genes, theta_pos=theta_pos, kind=kind, lognormal_mean=lognormal_mean)


class PoissonFactorization(nn.Module):
    """softplus(W) @ exp(F): base of PNMF / NSF2 / the hybrids; reference likelihoods.py:39-53.
    ``likelihood="nb"`` (here and on every count model below): negative-binomial noise with the per-gene parameter
    ``theta`` (raw; softplus(theta) = theta0 at the start) in place of Poisson noise."""

    def __init__(self, prior, y, L=10, likelihood="poisson", theta0=10.0):
        super().__init__()
        D, N = y.shape
        self.prior = prior
        self.W = nn.Parameter(torch.rand((D, L)))
        _init_likelihood(self, likelihood, theta0, D)

    def get_rate(self, prior_samples):
        return torch.matmul(torch.nn.functional.softplus(self.W), torch.exp(prior_samples))   # (E, D, N)


class PNMF(PoissonFactorization):
    """Non-spatial Poisson NMF over a GaussianPrior; reference likelihoods.py:56-72.  ``residuals`` is that of the spatial
    count models and ``likelihoods.model_residual_autocorr(model, X, y, ...)`` scores it as ``NSF.residual_autocorr`` scores
    an ``NSF``; the factors exist only for the fitted spots, so ``X`` (the coordinates of the fitted spots, or of those of
    ``idx`` after indexing) is used for the neighbour graph alone."""
    _residual_theta = _ResidualScores._residual_theta
    _residual_autocorr = _ResidualScores.residual_autocorr          # reached through model_residual_autocorr
    residuals = _ResidualScores.residuals

    def __init__(self, prior, y, L=10, likelihood="poisson", theta0=10.0):
        super().__init__(prior=prior, y=y, L=L, likelihood=likelihood, theta0=theta0)
        D, N = y.shape
        self.V = nn.Parameter(torch.ones((N,)))
        self.X = nn.Parameter(torch.zeros((N, 2)), requires_grad=False)

    def forward(self, E=10, **kwargs):
        qF, pF = self.prior()
        Z = self.get_rate(qF.rsample((E,)))
        pY = _count_dist(self, torch.nn.functional.softplus(self.V) * Z)
        return pY, qF, pF

    def expected_loglik(self, X, y, idx=None, E=10, eps=None, with_lgamma=True, **kwargs):
        """Fused form of ``forward``'s ``pY.log_prob(y).mean(0).sum()``: (E_q[log p(y | F)] as a scalar, qF, pF).  ``X`` is
        accepted for the signature of the spatial models and unused; ``y``: dense counts or a ``SparseCounts`` (for a
        batch, ``y[:, idx]`` together with ``idx``)."""
        qF, pF = self.prior() if idx is None else self.prior.forward_batched(idx)
        V = self.V if idx is None else self.V[idx]
        ll = _expected_loglik(self, [qF], [torch.nn.functional.softplus(self.W)], torch.nn.functional.softplus(V), y, E,
                              with_lgamma, eps)
        return ll, qF, pF

    def _residual_data(self, y, what):
        if isinstance(y, SparseExpression):
            raise TypeError(f"PNMF.{what}: a SparseExpression holds real-valued expression (values - offset), not counts; "
                            "pass the counts, dense or as a whole SparseCounts")
        if isinstance(y, SparseCounts) and y.base is not y:
            raise TypeError(f"PNMF.{what}: a view y[:, idx]; pass the whole SparseCounts of the scored spots")

    def _score_parts(self, X, idx, V, kwargs):
        _known_kwargs("PNMF", kwargs, ())
        Xb = X if idx is None else X[idx]
        qF = (self.prior() if idx is None else self.prior.forward_batched(idx))[0]
        if qF.mean.shape[-1] != Xb.shape[0]:
            raise ValueError(f"PNMF: the factors exist only for the fitted spots ({qF.mean.shape[-1]} here), so {Xb.shape[0]} "
                             "coordinates cannot be scored; X is used for the neighbour graph alone")
        Vp = _deviance_size_factors(self.V, idx, V, Xb.shape[0], type(self).__name__)
        return [qF], [torch.nn.functional.softplus(self.W)], Vp, Xb


class NSF2(PoissonFactorization, _ResidualScores):
    """Non-negative spatial factorisation over an SVGP prior; reference likelihoods.py:74-97."""

    def __init__(self, gp, y, L=10, likelihood="poisson", theta0=10.0):
        super().__init__(prior=gp, y=y, L=L, likelihood=likelihood, theta0=theta0)
        D, N = y.shape
        self.V = nn.Parameter(torch.ones((N,)))

    def forward(self, X, E=10, verbose=False, **kwargs):
        qF, qU, pU = self.prior(X=X, verbose=verbose, **kwargs)
        Z = self.get_rate(qF.rsample((E,)))
        pY = _count_dist(self, torch.nn.functional.softplus(self.V) * Z)
        return pY, qF, qU, pU

    def forward_batched(self, X, idx, E=10, verbose=False, **kwargs):
        qF, qU, pU = self.prior(X=X[idx], verbose=verbose, **kwargs)
        Z = self.get_rate(qF.rsample((E,)))
        pY = _count_dist(self, torch.nn.functional.softplus(self.V[idx]) * Z)
        return pY, qF, qU, pU

    def expected_loglik(self, X, y, idx=None, E=10, eps=None, with_lgamma=True, **kwargs):
        """Fused training-step form: (E_q[log p(y | F)] as a scalar, qF, qU, pU)."""
        Xb = X if idx is None else X[idx]
        V = self.V if idx is None else self.V[idx]
        qF, qU, pU = self.prior(X=Xb, **kwargs)
        ll = _expected_loglik(self, [qF], [torch.nn.functional.softplus(self.W)], torch.nn.functional.softplus(V), y, E,
                              with_lgamma, eps)
        return ll, qF, qU, pU

    def deviance(self, X, y, idx=None, V=None, lognormal_mean=True, family="poisson", theta=None, **kwargs):
        """Poisson deviance of ``y`` (D, B) at ``X`` (or ``X[idx]``) under the predictive mean rate: a ``PoissonDeviance``.
        ``V=None`` uses softplus(self.V) (indexed by ``idx``); held-out spots need explicit positive size factors.
        The same for ``likelihood="nb"``: the Poisson deviance of the mean rate is what the nsf paper reports for every
        likelihood.  ``family="nb"`` (or ``"model"`` on an NB model) scores under the negative binomial instead and returns
        an ``NBDeviance`` with theta = softplus(self.theta), or the positive ``theta=`` (a scalar or (D,))."""
        theta_pos = _deviance_theta(self, self.W, family, theta)
        with torch.no_grad():
            Xb = X if idx is None else X[idx]
            Vp = _deviance_size_factors(self.V, idx, V, Xb.shape[0], type(self).__name__)
            qF = self.prior(X=Xb, **kwargs)[0]
            return _deviance_of([qF], [torch.nn.functional.softplus(self.W)], Vp, theta_pos, y, lognormal_mean)

    def _score_parts(self, X, idx, V, kwargs):
        Xb = X if idx is None else X[idx]
        Vp = _deviance_size_factors(self.V, idx, V, Xb.shape[0], type(self).__name__)
        return [self.prior(X=Xb, **kwargs)[0]], [torch.nn.functional.softplus(self.W)], Vp, Xb


class NSF(nn.Module, _ResidualScores):
    """Same model with W, V held directly; reference likelihoods.py:227-268."""

    def __init__(self, gp, y, L=10, likelihood="poisson", theta0=10.0):
        super().__init__()
        D, N = y.shape
        self.gp = gp
        self.W = nn.Parameter(torch.rand((D, L)))
        self.V = nn.Parameter(torch.ones((N,)))
        _init_likelihood(self, likelihood, theta0, D)

    def _rate(self, qF, V, E):
        F = torch.exp(qF.rsample((E,)))
        return V * torch.matmul(torch.nn.functional.softplus(self.W), F)

    def forward(self, X, E=10, verbose=False, **kwargs):
        qF, qU, pU = self.gp(X=X, verbose=verbose, **kwargs)
        return _count_dist(self, self._rate(qF, torch.nn.functional.softplus(self.V), E)), qF, qU, pU

    def forward_batched(self, X, idx, E=10, verbose=False, **kwargs):
        qF, qU, pU = self.gp(X=X[idx], verbose=verbose, **kwargs)
        return _count_dist(self, self._rate(qF, torch.nn.functional.softplus(self.V)[idx], E)), qF, qU, pU

    def expected_loglik(self, X, y, idx=None, E=10, eps=None, with_lgamma=True, **kwargs):
        Xb = X if idx is None else X[idx]
        V = torch.nn.functional.softplus(self.V)
        qF, qU, pU = self.gp(X=Xb, **kwargs)
        ll = _expected_loglik(self, [qF], [torch.nn.functional.softplus(self.W)], V if idx is None else V[idx], y, E,
                              with_lgamma, eps)
        return ll, qF, qU, pU

    def deviance(self, X, y, idx=None, V=None, lognormal_mean=True, family="poisson", theta=None, **kwargs):
        """Poisson deviance of ``y`` (D, B) at ``X`` (or ``X[idx]``) under the predictive mean rate: a ``PoissonDeviance``.
        ``V=None`` uses softplus(self.V) (indexed by ``idx``); held-out spots need explicit positive size factors.
        The same for ``likelihood="nb"``: the Poisson deviance of the mean rate is what the nsf paper reports for every
        likelihood.  ``family="nb"`` (or ``"model"`` on an NB model) scores under the negative binomial instead and returns
        an ``NBDeviance`` with theta = softplus(self.theta), or the positive ``theta=`` (a scalar or (D,))."""
        theta_pos = _deviance_theta(self, self.W, family, theta)
        with torch.no_grad():
            Xb = X if idx is None else X[idx]
            Vp = _deviance_size_factors(self.V, idx, V, Xb.shape[0], type(self).__name__)
            qF = self.gp(X=Xb, **kwargs)[0]
            return _deviance_of([qF], [torch.nn.functional.softplus(self.W)], Vp, theta_pos, y, lognormal_mean)

    def _score_parts(self, X, idx, V, kwargs):
        Xb = X if idx is None else X[idx]
        Vp = _deviance_size_factors(self.V, idx, V, Xb.shape[0], type(self).__name__)
        return [self.gp(X=Xb, **kwargs)[0]], [torch.nn.functional.softplus(self.W)], Vp, Xb


class MGGP_NSF(NSF):
    """NSF over a multi-group GP (groupsX is positional); reference likelihoods.py:341-374."""

    def _gp(self, X, groupsX, verbose):
        if getattr(self.gp, "_whitened", False):
            return self.gp(X, verbose=verbose, groupsX=groupsX)     # MGGP_WSVGP takes groupsX as a keyword
        return self.gp(X, groupsX, verbose)

    def forward(self, X, groupsX, E=10, verbose=False):
        qF, qU, pU = self._gp(X, groupsX, verbose)
        return _count_dist(self, self._rate(qF, torch.nn.functional.softplus(self.V), E)), qF, qU, pU

    def forward_batched(self, X, groupsX, idx, E=10, verbose=False):
        qF, qU, pU = self._gp(X[idx], groupsX[idx], verbose)
        return _count_dist(self, self._rate(qF, torch.nn.functional.softplus(self.V)[idx], E)), qF, qU, pU

    def expected_loglik(self, X, y, groupsX=None, idx=None, E=10, eps=None, with_lgamma=True, **kwargs):
        """Fused training-step form; the group ids follow the sampled spots (``groupsX[idx]``, as in
        ``forward_batched`` / reference likelihoods.py:364-366)."""
        if groupsX is None:
            raise TypeError("MGGP_NSF.expected_loglik needs groupsX")
        Xb, gb = (X, groupsX) if idx is None else (X[idx], groupsX[idx])
        V = torch.nn.functional.softplus(self.V)
        qF, qU, pU = self._gp(Xb, gb, False)
        ll = _expected_loglik(self, [qF], [torch.nn.functional.softplus(self.W)], V if idx is None else V[idx], y, E,
                              with_lgamma, eps)
        return ll, qF, qU, pU

    def deviance(self, X, y, groupsX=None, idx=None, V=None, lognormal_mean=True, family="poisson", theta=None, **kwargs):
        """``NSF.deviance`` with the group ids of the spots being scored (``groupsX[idx]`` with ``idx``)."""
        if groupsX is None:
            raise TypeError("MGGP_NSF.deviance needs groupsX")
        theta_pos = _deviance_theta(self, self.W, family, theta)
        with torch.no_grad():
            Xb, gb = (X, groupsX) if idx is None else (X[idx], groupsX[idx])
            Vp = _deviance_size_factors(self.V, idx, V, Xb.shape[0], type(self).__name__)
            qF = self._gp(Xb, gb, False)[0]
            return _deviance_of([qF], [torch.nn.functional.softplus(self.W)], Vp, theta_pos, y, lognormal_mean)

    def _score_parts(self, X, idx, V, kwargs):
        groupsX = kwargs.get("groupsX")
        if groupsX is None:
            raise TypeError("MGGP_NSF.residual_autocorr and MGGP_NSF.residuals need groupsX=")
        Xb, gb = (X, groupsX) if idx is None else (X[idx], groupsX[idx])
        Vp = _deviance_size_factors(self.V, idx, V, Xb.shape[0], type(self).__name__)
        return [self._gp(Xb, gb, False)[0]], [torch.nn.functional.softplus(self.W)], Vp, Xb


class Hybrid_NSF2(nn.Module, _ResidualScores):
    """Spatial (GP) + non-spatial (GaussianPrior) factors; reference likelihoods.py:100-164."""

    def __init__(self, gp, prior, y, L=10, T=10, likelihood="poisson", theta0=10.0):
        super().__init__()
        D, N = y.shape
        self.sf = PoissonFactorization(prior=gp, y=y, L=L)
        self.cf = PoissonFactorization(prior=prior, y=y, L=T)
        self.V = nn.Parameter(torch.ones((N,)))
        _init_likelihood(self, likelihood, theta0, D)      # one theta per gene for the sum of both factor sets

    def _pY(self, qF1, qF2, V, E):
        Z = self.sf.get_rate(qF1.rsample((E,))) + self.cf.get_rate(qF2.rsample((E,)))
        return _count_dist(self, V * Z)

    def forward(self, X, E=10, verbose=False, **kwargs):
        qF1, qU, pU = self.sf.prior(X=X, verbose=verbose, **kwargs)
        qF2, pF2 = self.cf.prior()
        return self._pY(qF1, qF2, torch.nn.functional.softplus(self.V), E), qF1, qU, pU, qF2, pF2

    def forward_batched(self, X, idx, E=10, verbose=False, **kwargs):
        qF1, qU, pU = self.sf.prior(X=X[idx], verbose=verbose, **kwargs)
        qF2, pF2 = self.cf.prior.forward_batched(idx)
        return self._pY(qF1, qF2, torch.nn.functional.softplus(self.V[idx]), E), qF1, qU, pU, qF2, pF2

    def forward_precomputed(self, W, idx, E=10, verbose=False, **kwargs):
        qF1, qU, pU = self.sf.prior.forward_precomputed(W, verbose=verbose, **kwargs)
        qF2, pF2 = self.cf.prior.forward_batched(idx)
        return self._pY(qF1, qF2, torch.nn.functional.softplus(self.V[idx]), E), qF1, qU, pU, qF2, pF2

    def expected_loglik(self, X, y, idx=None, E=10, eps=None, with_lgamma=True, **kwargs):
        Xb = X if idx is None else X[idx]
        V = self.V if idx is None else self.V[idx]
        qF1, qU, pU = self.sf.prior(X=Xb, **kwargs)
        qF2, pF2 = self.cf.prior() if idx is None else self.cf.prior.forward_batched(idx)
        sp = torch.nn.functional.softplus
        ll = _expected_loglik(self, [qF1, qF2], [sp(self.sf.W), sp(self.cf.W)], sp(V), y, E, with_lgamma, eps)
        return ll, qF1, qU, pU, qF2, pF2

    def deviance(self, X, y, idx=None, V=None, lognormal_mean=True, family="poisson", theta=None, **kwargs):
        """Poisson deviance of ``y`` (D, B) at ``X`` (or ``X[idx]``) under the predictive mean rate of both factor sets: a
        ``PoissonDeviance``.  The non-spatial factors exist only for the fitted spots: other spots raise ValueError.
        ``family`` and ``theta`` as in ``NSF.deviance``."""
        theta_pos = _deviance_theta(self, self.sf.W, family, theta)
        with torch.no_grad():
            Xb = X if idx is None else X[idx]
            _hybrid_spots(self.V.shape[0], Xb.shape[0], idx, V, type(self).__name__)
            Vp = _deviance_size_factors(self.V, idx, V, Xb.shape[0], type(self).__name__)
            qF1 = self.sf.prior(X=Xb, **kwargs)[0]
            qF2 = (self.cf.prior() if idx is None else self.cf.prior.forward_batched(idx))[0]
            sp = torch.nn.functional.softplus
            return _deviance_of([qF1, qF2], [sp(self.sf.W), sp(self.cf.W)], Vp, theta_pos, y, lognormal_mean)

    def _score_parts(self, X, idx, V, kwargs):
        Xb = X if idx is None else X[idx]
        _hybrid_spots(self.V.shape[0], Xb.shape[0], idx, V, type(self).__name__)
        Vp = _deviance_size_factors(self.V, idx, V, Xb.shape[0], type(self).__name__)
        qF1 = self.sf.prior(X=Xb, **kwargs)[0]
        qF2 = (self.cf.prior() if idx is None else self.cf.prior.forward_batched(idx))[0]
        sp = torch.nn.functional.softplus
        return [qF1, qF2], [sp(self.sf.W), sp(self.cf.W)], Vp, Xb


class Hybrid_NSF_Exact(Hybrid_NSF2):
    """Hybrid model with the log-normal mean exp(m + s^2/2) in place of sampling; reference
    likelihoods.py:167-222.  Nothing is sampled, so the rate has NO sample axis: ``pY.rate`` is (D,N) and ``E`` is
    ignored, as in the reference."""

    def _pY(self, qF1, qF2, V, E):
        Z = self.sf.get_rate(qF1.mean + 0.5 * qF1.scale ** 2) + self.cf.get_rate(qF2.mean + 0.5 * qF2.scale ** 2)
        return _count_dist(self, V * Z)

    def expected_loglik(self, X, y, idx=None, E=10, eps=None, with_lgamma=True, **kwargs):
        """The closed-form objective of THIS class as the reference's loops evaluate it -- not the sampled one of
        Hybrid_NSF2.  With a (D,N) rate, ``pY.log_prob(y).mean(axis=0).sum()`` (utilities.py:537) and
        ``(y log r - r).mean(axis=0).sum()`` (utilities.py:508-510) average over the GENE axis: the value is
        (1/D) sum_dn log Poisson(y | V (W1 exp(m1 + s1^2/2) + W2 exp(m2 + s2^2/2))).  Evaluated by the fused kernel as
        one noise-free "sample" of F = m + s^2/2 (gpz_poisson_nsf; the chain to m and s runs through torch);
        ``E`` and ``eps`` are accepted and unused."""
        Xb = X if idx is None else X[idx]
        V = self.V if idx is None else self.V[idx]
        qF1, qU, pU = self.sf.prior(X=Xb, **kwargs)
        qF2, pF2 = self.cf.prior() if idx is None else self.cf.prior.forward_batched(idx)
        sp = torch.nn.functional.softplus
        m = torch.cat([qF1.mean + 0.5 * qF1.scale ** 2, qF2.mean + 0.5 * qF2.scale ** 2], dim=0)
        zero = torch.zeros_like(m)
        Wc = torch.cat([sp(self.sf.W), sp(self.cf.W)], dim=1)
        if self.likelihood == "nb":
            ll = _nb_loglik_function(y).apply(m, zero, Wc, sp(V), sp(self.theta), zero[None], y, with_lgamma)
        else:
            ll = _loglik_function(y).apply(m, zero, Wc, sp(V), zero[None], y, with_lgamma)
        return ll / y.shape[0], qF1, qU, pU, qF2, pF2


class Hybrid_NSF(NSF):
    """NSF plus mean-field non-spatial factors held in the module (raw, un-soft-plussed loadings);
    reference likelihoods.py:271-338."""

    def __init__(self, gp, y, L=10, non_spatial_factors=10, likelihood="poisson", theta0=10.0):
        super().__init__(gp=gp, y=y, L=L, likelihood=likelihood, theta0=theta0)
        D, N = y.shape
        self.W2 = nn.Parameter(torch.rand((D, non_spatial_factors)))
        self.mF = nn.Parameter(torch.zeros((non_spatial_factors, N)))
        self.scale_qF = nn.Parameter(1e-1 * torch.rand((non_spatial_factors, N)))

    def _hybrid(self, qF, mF, raw_scale, V, E):
        scale2 = torch.nn.functional.softplus(raw_scale)
        qF2 = _dist(distributions.Normal, mF, scale2)
        F = torch.exp(torch.cat((qF.rsample((E,)), qF2.rsample((E,))), dim=1))
        Z = torch.matmul(torch.cat((self.W, self.W2), dim=1), F)
        pF2 = _dist(distributions.Normal, torch.zeros_like(mF), torch.ones_like(scale2))
        return _count_dist(self, V * Z), qF2, pF2

    def forward(self, X, E=10, verbose=False, **kwargs):
        qF, qU, pU = self.gp(X=X, verbose=verbose, **kwargs)
        pY, qF2, pF2 = self._hybrid(qF, self.mF, self.scale_qF, torch.nn.functional.softplus(self.V), E)
        return pY, qF, qU, pU, qF2, pF2

    def forward_batched(self, X, idx, E=10, verbose=False, **kwargs):
        qF, qU, pU = self.gp(X=X[idx], verbose=verbose, **kwargs)
        pY, qF2, pF2 = self._hybrid(qF, self.mF[:, idx], self.scale_qF[:, idx],
                                    torch.nn.functional.softplus(self.V)[idx], E)
        return pY, qF, qU, pU, qF2, pF2

    def expected_loglik(self, X, y, idx=None, E=10, eps=None, with_lgamma=True, **kwargs):
        """Fused training-step form over both factor sets (raw loadings W, W2 as in ``_hybrid``)."""
        Xb = X if idx is None else X[idx]
        mF, rs = (self.mF, self.scale_qF) if idx is None else (self.mF[:, idx], self.scale_qF[:, idx])
        V = torch.nn.functional.softplus(self.V)
        qF, qU, pU = self.gp(X=Xb, **kwargs)
        scale2 = torch.nn.functional.softplus(rs)
        qF2 = _dist(distributions.Normal, mF, scale2)
        pF2 = _dist(distributions.Normal, torch.zeros_like(mF), torch.ones_like(scale2))
        ll = _expected_loglik(self, [qF, qF2], [self.W, self.W2], V if idx is None else V[idx], y, E, with_lgamma, eps)
        return ll, qF, qU, pU, qF2, pF2

    def deviance(self, X, y, idx=None, V=None, lognormal_mean=True, family="poisson", theta=None, **kwargs):
        """Poisson deviance of ``y`` (D, B) at ``X`` (or ``X[idx]``) under the predictive mean rate of both factor sets (raw
        loadings W, W2 as in ``_hybrid``).  The non-spatial factors exist only for the fitted spots: other spots raise
        ValueError.  ``family`` and ``theta`` as in ``NSF.deviance``."""
        theta_pos = _deviance_theta(self, self.W, family, theta)
        with torch.no_grad():
            Xb = X if idx is None else X[idx]
            _hybrid_spots(self.V.shape[0], Xb.shape[0], idx, V, type(self).__name__)
            Vp = _deviance_size_factors(self.V, idx, V, Xb.shape[0], type(self).__name__)
            mF, rs = (self.mF, self.scale_qF) if idx is None else (self.mF[:, idx], self.scale_qF[:, idx])
            qF = self.gp(X=Xb, **kwargs)[0]
            qF2 = distributions.Normal(mF, torch.nn.functional.softplus(rs), validate_args=False)
            return _deviance_of([qF, qF2], [self.W, self.W2], Vp, theta_pos, y, lognormal_mean)

    def _score_parts(self, X, idx, V, kwargs):
        Xb = X if idx is None else X[idx]
        _hybrid_spots(self.V.shape[0], Xb.shape[0], idx, V, type(self).__name__)
        Vp = _deviance_size_factors(self.V, idx, V, Xb.shape[0], type(self).__name__)
        mF, rs = (self.mF, self.scale_qF) if idx is None else (self.mF[:, idx], self.scale_qF[:, idx])
        qF2 = distributions.Normal(mF, torch.nn.functional.softplus(rs), validate_args=False)
        return [self.gp(X=Xb, **kwargs)[0], qF2], [self.W, self.W2], Vp, Xb


# --------------------------------------------------------------------------------------------
# Gaussian factor models on normalised, real-valued expression: RSF (a GP prior on the factors; the nsf paper's
# real-valued spatial factorisation, which it shows to be MEFISTO's model) and FA (an i.i.d. prior).  W is real and
# there is no link, so E_q[log p(y | F)] is a closed form: `expected_loglik` is exact, takes no samples and runs the
# fused gpz_gaussian_fa step.
# --------------------------------------------------------------------------------------------

class _GaussianFALogLik(torch.autograd.Function):
    """E_q[sum_dn log Normal(y | b + W F, noise_sd)] through gpz_gaussian_fa (value and gradients in one fused step;
    backward only scales them)."""

    @staticmethod
    def forward(ctx, mean, scale, W, b, noise_sd, y):
        from . import ops
        ll, _, dmean, dscale, dW, db, dsd = ops.gaussian_fa(mean, scale, W, b, noise_sd, y)
        ctx.save_for_backward(dmean.to(mean.dtype), dscale.to(scale.dtype), dW.to(W.dtype), db.to(b.dtype),
                              dsd.to(noise_sd.dtype))
        return ll.to(mean.dtype)

    @staticmethod
    def backward(ctx, g):
        dmean, dscale, dW, db, dsd = ctx.saved_tensors
        return g * dmean, g * dscale, g * dW, g * db, g * dsd, None


class _SparseGaussianFALogLik(torch.autograd.Function):
    """_GaussianFALogLik for a SparseExpression (or its view y[:, idx]) through gpz_gaussian_fa_sparse."""

    @staticmethod
    def forward(ctx, mean, scale, W, b, noise_sd, y):
        from . import ops
        ll, _, _, dmean, dscale, dW, db, dsd = ops.gaussian_fa_sparse(mean, scale, W, b, noise_sd, y)
        ctx.save_for_backward(dmean.to(mean.dtype), dscale.to(scale.dtype), dW.to(W.dtype), db.to(b.dtype),
                              dsd.to(noise_sd.dtype))
        return ll.to(mean.dtype)

    @staticmethod
    def backward(ctx, g):
        dmean, dscale, dW, db, dsd = ctx.saved_tensors
        return g * dmean, g * dscale, g * dW, g * db, g * dsd, None


def _gaussian_loglik_function(y):
    """The autograd function of the fused Gaussian step for this form of the data (``_loglik_function``'s sibling)."""
    return _SparseGaussianFALogLik if isinstance(y, SparseExpression) else _GaussianFALogLik


def gaussian_expected_loglik(qF_list, W_list, b, noise_sd, y):
    """Exact E_q[log p(y | F)] for y ~ Normal(b[:, None] + sum_k W_k F_k, noise_sd[:, None]), F_k ~ qF_k independent.

    qF_list: Normal distributions over (L_k, N) factors; W_list: real (D, L_k) loadings; b (D,); noise_sd (D,) positive
    standard deviations; y: the (D, N) data, dense (gpz_gaussian_fa) or a ``SparseExpression`` / its view ``y[:, idx]``
    (gpz_gaussian_fa_sparse).  Differentiable in every argument but y."""
    mean = torch.cat([q.mean for q in qF_list], dim=0)
    scale = torch.cat([q.scale for q in qF_list], dim=0)
    W = torch.cat(list(W_list), dim=1)
    return _gaussian_loglik_function(y).apply(mean, scale, W, b, noise_sd, y)


class GaussianScore(NamedTuple):
    """What ``RSF.score`` / ``FA.score`` return; every tensor is fp64 and carries no graph.  ``sse_per_gene`` is the squared
    error of the predictive mean b + W E_q[F] and ``mse_per_gene`` = sse / B, ``mse`` = sum sse / (D B);
    ``r2_per_gene`` = 1 - sse / sum_n (y - mean_n y)^2 (NaN where that sum is 0) and ``r2`` the same over all genes.
    ``loglik`` is the EXPECTED log density under q(F): next to the squared error it carries sum_l W[d,l]^2 sum_n scale^2,
    the variance of q(F), so it is not a function of ``sse`` alone."""
    loglik: torch.Tensor
    sse_per_gene: torch.Tensor
    mse_per_gene: torch.Tensor
    mse: torch.Tensor
    r2_per_gene: torch.Tensor
    r2: torch.Tensor


def gaussian_score(qF_list, W_list, b, noise_sd, y):
    """``GaussianScore`` of the dense (D, B) data ``y`` from the value-only form of gpz_gaussian_fa (one pass over y); the
    null sums of squares come from a plain torch reduction of y in fp64.  Of a ``SparseExpression`` (or its view): the
    value-only form of gpz_gaussian_fa_sparse, which returns the null sums of squares itself (``ss_per_gene``)."""
    from . import ops
    with torch.no_grad():
        mean = torch.cat([q.mean for q in qF_list], dim=0)
        scale = torch.cat([q.scale for q in qF_list], dim=0)
        W = torch.cat(list(W_list), dim=1)
        D, B = y.shape
        if isinstance(y, SparseExpression):
            ll, sse, null = ops.gaussian_fa_sparse(mean, scale, W, b, noise_sd, y, grads=False)
        else:
            ll, sse = ops.gaussian_fa(mean, scale, W, b, noise_sd, y, grads=False)
            yd = y.detach().double()
            null = ((yd - yd.mean(dim=1, keepdim=True)) ** 2).sum(dim=1)
        return GaussianScore(loglik=ll.clone(), sse_per_gene=sse, mse_per_gene=sse / B, mse=sse.sum() / (D * B),
                             r2_per_gene=_explained(sse, null), r2=_explained(sse.sum(), null.sum()))


def gaussian_residual_autocorr(qF_list, W_list, b, noise_sd, y, nbr, *, kind="pearson", slab_genes=0, mode="moran",
                               assumption="normality", n_perms=None, seed=0, perms=None, return_sims=False):
    """``residual_autocorr`` for the Gaussian factor models (``RSF``, ``FA``): the spatial autocorrelation of every gene's
    residuals under the predictive mean yhat = b[:, None] + sum_k W_k E_q[F_k] over the neighbour table ``nbr`` (B, K) of the
    B scored spots.  ``noise_sd`` (D,) positive, inside ``NOISE_SD_RANGE``.  ``y``: dense (D, B) or a whole
    ``SparseExpression`` (the same bits as on ``y.to_dense()``).  ``kind``: "pearson" (default), (y - yhat) / noise_sd;
    "response", y - yhat in data units, for plotting; "predictive", (y - yhat) / sqrt(noise_sd^2 + W^2 scale^2), which
    stays a standardisation at held-out spots, where q(F) is wide.  "deviance" raises ValueError: for a Gaussian the signed
    square root of the unit deviance is the Pearson residual.  I and C do not change under a per-gene affine map, so
    "pearson" and "response" give the same I and C up to fp32 rounding and differ in ``residual_mean``, ``residual_var`` and
    the maps; "predictive" differs spot by spot and gives another I.

    ``mode``, ``assumption``, ``n_perms``, ``seed``, ``perms`` and ``return_sims`` as in ``residual_autocorr``, and the same
    return types; with all of them at their defaults a ``ResidualAutocorr``.  Neither the (D, B) mean nor the residuals are
    materialised (``ops.gaussian_residual_stats`` / ``ops.gaussian_residual_autocorr_perm``).  Like the count form, the null
    ignores the degrees of freedom the fit used: the score ranks genes, it is not a calibrated test."""
    from . import ops
    who = "gaussian_residual_autocorr"
    ops._gaussian_kind(who, kind)
    ops._gaussian_data(who, y)
    B = int(nbr.shape[0]) if isinstance(nbr, torch.Tensor) else len(nbr)
    null = _residual_null_args(who, B, mode, assumption, n_perms, perms)
    nbr = torch.as_tensor(nbr)
    entries = _gaussian_entries(b, noise_sd, y, nbr, kind, slab_genes, mode, return_sims)
    return _residual_autocorr_checked(entries, qF_list, W_list, nbr, null, mode, assumption, seed)


def _gaussian_entries(b, noise_sd, y, nbr, kind, slab_genes, mode, return_sims):
    """The Gaussian family for ``_residual_autocorr_checked``: no Moran-only entry, the wide and the permutation entry."""
    from . import ops

    def bind(mean, scale, W):
        head = (mean, scale, W, b, noise_sd, y, nbr)
        return (None, lambda: ops.gaussian_residual_stats(*head, None, kind, slab_genes),
                lambda perms: ops.gaussian_residual_autocorr_perm(*head, perms, None, kind, stat=mode, return_sims=return_sims,
                                                                  slab_genes=slab_genes))
    return bind


def gaussian_residuals(qF_list, W_list, b, noise_sd, y, genes, *, kind="pearson"):
    """(len(genes), B) fp32 residuals of the listed genes, gene-major like ``y``, under the predictive mean of
    ``gaussian_residual_autocorr``: one gene's residual map for plotting (``kind="response"`` is in data units).
    ``genes``: gene indices in any order, repeats allowed."""
    from . import ops
    if genes is None:
        raise ValueError("gaussian_residuals: genes (a list of gene indices) needed; the full (D, B) array is what this avoids")
    with torch.no_grad():
        mean, scale, W = _cat_factors(qF_list, W_list)
        return ops.gaussian_residuals(mean, scale, W, b, noise_sd, y, genes, kind).T.contiguous()


def model_residual_autocorr(model, X, y, idx=None, **keywords):
    """Is spatial structure left in what ``model`` did not explain, and in which genes -- one call for every model of the
    zoo, so that a non-spatial fit (``FA``, ``PNMF``) stands next to a spatial one (``RSF``, ``NSF``) on the same data.  For
    the count models with a GP prior it is ``model.residual_autocorr(X, y, idx, ...)``; ``PNMF`` is scored by the same code
    (keywords as there: ``V``, ``kind``, ``family``, ``theta``, ...); ``RSF`` and ``FA`` by the Gaussian form below
    (``kind`` "pearson", "response" or "predictive", ``n_neighs``, ``graph``, ``mode``, ``assumption``, ``n_perms``, ``seed``,
    ``perms``, ``return_sims``, and ``groupsX`` for an ``RSF`` over a multi-group GP).  Returns what ``residual_autocorr``
    returns.  ``RSF`` takes q(F) from its GP at ``X[idx]``, so held-out spots work; the factors of ``FA`` and ``PNMF`` exist
    only for the fitted spots, where ``X`` is used for the neighbour graph alone."""
    fn = getattr(model, "residual_autocorr", None) or getattr(model, "_residual_autocorr", None)
    if fn is None:
        raise TypeError(f"model_residual_autocorr: {type(model).__name__} has no residual diagnostic")
    return fn(X, y, idx, **keywords)


class _GaussianResidualScores:
    """``_residual_autocorr`` (behind ``model_residual_autocorr``) and ``residuals`` of the Gaussian factor models.  A model supplies
    ``_residual_factors(X, idx, groupsX)`` -> q(F) at the scored spots."""

    def _scored_spots(self, what, X, y, idx, kind):
        """The refusals that need no device, and the number of scored spots (the rows of ``X[idx]``)."""
        from . import ops
        who = f"{type(self).__name__}.{what}"
        ops._gaussian_kind(who, kind)
        ops._gaussian_data(who, y)
        return who, _scored_spot_count(X, idx)

    def _residual_autocorr(self, X, y, idx=None, *, kind="pearson", n_neighs=6, graph=None, mode="moran", assumption="normality",
                           n_perms=None, seed=0, perms=None, return_sims=False, groupsX=None):
        """Is spatial structure left in what the fit did not explain, and in which genes: Moran's I (or Geary's C) of every
        gene's residuals at ``X`` (or ``X[idx]``) over the scored spots' ``n_neighs``-nearest-neighbour graph
        (``ops.spatial_knn``), or over ``graph=``, a (B, K) table.  ``y`` (D, B) dense or a whole ``SparseExpression`` of the
        scored spots.  ``kind`` ("pearson", "response", "predictive"), ``mode``, ``assumption``, ``n_perms``, ``seed``,
        ``perms`` and ``return_sims`` as in ``likelihoods.gaussian_residual_autocorr``; with all of them at their defaults the
        result is a ``ResidualAutocorr``.  The residual Moran's I of a non-spatial fit (``FA``) next to a spatial one
        (``RSF``) on the same data is the comparison the spatial prior is judged by."""
        from . import ops
        who, B = self._scored_spots("residual_autocorr", X, y, idx, kind)
        null = _residual_null_args(who, B, mode, assumption, n_perms, perms)
        with torch.no_grad():
            qF = self._residual_factors(X, idx, groupsX)
            nbr = ops.spatial_knn(X if idx is None else X[idx], int(n_neighs)) if graph is None else torch.as_tensor(graph)
            entries = _gaussian_entries(self.b, _noise_sd(self.noise), y, nbr, kind, 0, mode, return_sims)
            return _residual_autocorr_checked(entries, [qF], [self.W], nbr, null, mode, assumption, seed)

    def residuals(self, X, y, genes, idx=None, *, kind="pearson", groupsX=None):
        """(len(genes), B) fp32 residuals of the listed genes at ``X`` (or ``X[idx]``): the rows ``model_residual_autocorr``
        scores.  Arguments as there."""
        self._scored_spots("residuals", X, y, idx, kind)
        with torch.no_grad():
            qF = self._residual_factors(X, idx, groupsX)
            return gaussian_residuals([qF], [self.W], self.b, _noise_sd(self.noise), y, genes, kind=kind)


def _call_gp(gp, X, groupsX=None):
    """q(F), q(U), p(U) of a GP at X; the multi-group GPs take the group ids as ``MGGP_NSF`` passes them."""
    if groupsX is None:
        return gp(X)
    if getattr(gp, "_whitened", False):
        return gp(X, groupsX=groupsX)          # MGGP_WSVGP takes groupsX as a keyword
    return gp(X, groupsX)


NOISE_SD_RANGE = (1e-18, 1e18)     # what gpz_gaussian_fa supports (include/gpzoo_hip.h): 1 / sd^2 must be a finite fp32


def _noise_sd(raw):
    """softplus(raw) kept inside the range the fused step supports: training may push the raw parameter anywhere, and a
    softplus that underflows would make 1 / sd^2 infinite in fp32."""
    return torch.nn.functional.softplus(raw).clamp(*NOISE_SD_RANGE)


def _known_kwargs(who, kwargs, known):
    """Keyword arguments are forwarded by the training loops (``groupsX=``); anything else is a mistake, not ignored."""
    extra = sorted(set(kwargs) - set(known))
    if extra:
        raise TypeError(f"{who}: unexpected keyword argument(s) {extra} (known: {sorted(known)})")


def _init_gaussian(module, y, L, noise0):
    """Parameters of the Gaussian factor models: W (D, L) real = randn / sqrt(L), b (D,) = the row means of y, noise (D,)
    raw with softplus(noise) = the row standard deviations of y floored at 1e-3, or the positive scalar ``noise0``.
    Of a whole ``SparseExpression`` the means and standard deviations come from fp64 segment sums over the stored
    entries (the offset shifts the mean and cancels in the deviation); nothing is densified."""
    import numpy as np
    from .utilities import init_softplus
    D, N = y.shape
    dt = torch.get_default_dtype()
    if isinstance(y, SparseExpression):
        if y.is_view:
            raise TypeError(f"{type(module).__name__}: built from a view y[:, idx]; pass the whole SparseExpression")
        s1, s2 = _gene_moments(y)
        row_mean = s1 / N - y.offset
        row_sd = (s2 / N - (s1 / N) ** 2).clamp_min(0.0).sqrt()
    else:
        yd = torch.as_tensor(y).detach().double()
        row_mean = yd.mean(dim=1)
        row_sd = None
    module.W = nn.Parameter(torch.randn((D, L)) / float(L) ** 0.5)
    module.b = nn.Parameter(row_mean.to(dtype=dt, device="cpu"))
    if noise0 is None:
        sd = (yd.std(dim=1, unbiased=False) if row_sd is None else row_sd).clamp_min(1e-3).cpu().numpy()
    else:
        if not float(noise0) > 0:
            raise ValueError(f"{type(module).__name__}: noise0 must be positive, got {noise0}")
        sd = np.full((D,), float(noise0), dtype=np.float64)
    module.noise = nn.Parameter(torch.as_tensor(init_softplus(sd), dtype=dt))


class _DenseNormal(distributions.Normal):
    """torch's Normal as ``RSF`` / ``FA`` return it from ``forward``: the sampled (E, D, N) form has no sparse evaluation, so
    ``log_prob`` of a ``SparseExpression`` raises TypeError instead of torch's message about a non-tensor value."""

    def log_prob(self, value):
        if isinstance(value, (SparseExpression, SparseCounts)):
            raise TypeError(f"pY.log_prob: a {type(value).__name__} goes through the fused step only "
                            "(model.expected_loglik / model.score); the sampled form needs the dense array, y.to_dense()")
        return super().log_prob(value)


class RSF(nn.Module, _GaussianResidualScores):
    """Real-valued spatial factorisation: y ~ Normal(b[:, None] + W F, softplus(noise)[:, None]) with a GP prior on the
    rows of F (``gp``: SVGP, WSVGP, VNNGP or, with ``groupsX=``, a multi-group GP) -- the nsf paper's RSF, i.e. MEFISTO.
    ``W`` (D, L) is real (``signed_loadings``: the training loops do not clamp it), ``b`` (D,) the intercept, ``noise`` (D,)
    raw: softplus(noise) is the per-gene noise standard deviation, as in ``GaussianLikelihood`` (kept inside
    ``NOISE_SD_RANGE``).  ``groupsX=`` is the only extra keyword the methods take; any other raises TypeError."""
    signed_loadings = True

    def __init__(self, gp, y, L=10, noise0=None):
        super().__init__()
        self.gp = gp
        _init_gaussian(self, y, L, noise0)

    def _pY(self, qF, E):
        sd = _noise_sd(self.noise)
        return _dist(_DenseNormal, self.b[:, None] + torch.matmul(self.W, qF.rsample((E,))), sd[:, None])

    def _qF(self, X, idx, kwargs):
        _known_kwargs("RSF", kwargs, ("groupsX",))
        gX = kwargs.get("groupsX")
        if idx is not None:
            X, gX = X[idx], (None if gX is None else gX[idx])
        return _call_gp(self.gp, X, gX)

    def forward(self, X, E=10, verbose=False, **kwargs):
        qF, qU, pU = self._qF(X, None, kwargs)
        return self._pY(qF, E), qF, qU, pU

    def forward_batched(self, X, idx, E=10, verbose=False, **kwargs):
        qF, qU, pU = self._qF(X, idx, kwargs)
        return self._pY(qF, E), qF, qU, pU

    def expected_loglik(self, X, y, idx=None, E=None, **kwargs):
        """Fused training-step form: (E_q[log p(y | F)] as a scalar, qF, qU, pU).  The value is exact -- what
        ``forward``'s ``pY.log_prob(y).mean(0).sum()`` estimates -- so ``E`` is accepted and unused.  For a batch pass
        ``y[:, idx]`` together with ``idx``; group ids (``groupsX=``) follow the sampled spots."""
        qF, qU, pU = self._qF(X, idx, kwargs)
        ll = gaussian_expected_loglik([qF], [self.W], self.b, _noise_sd(self.noise), y)
        return ll, qF, qU, pU

    def score(self, X, y, idx=None, **kwargs):
        """``GaussianScore`` of ``y`` (D, B) at ``X`` (or ``X[idx]``), held-out spots included: the squared error and R^2 of
        the predictive mean, and the expected log density (which also carries the variance of q(F))."""
        with torch.no_grad():
            qF = self._qF(X, idx, kwargs)[0]
            return gaussian_score([qF], [self.W], self.b, _noise_sd(self.noise), y)

    def _residual_factors(self, X, idx, groupsX):
        """q(F) from the GP at ``X[idx]``, held-out spots included, as in ``score``."""
        return self._qF(X, idx, {} if groupsX is None else {"groupsX": groupsX})[0]


class FA(nn.Module, _GaussianResidualScores):
    """Factor analysis: ``RSF``'s likelihood over a ``GaussianPrior`` (i.i.d. factors per spot), with ``PNMF``'s return
    tuples ``(..., qF, pF)``."""
    signed_loadings = True

    def __init__(self, prior, y, L=10, noise0=None):
        super().__init__()
        self.prior = prior
        _init_gaussian(self, y, L, noise0)

    _pY = RSF._pY

    def forward(self, E=10, **kwargs):
        _known_kwargs("FA", kwargs, ("X", "verbose"))       # the loops call model(X=X, E=E); the factors are per spot
        qF, pF = self.prior()
        return self._pY(qF, E), qF, pF

    def forward_batched(self, idx, E=10, **kwargs):
        _known_kwargs("FA", kwargs, ("X", "verbose"))
        qF, pF = self.prior.forward_batched(idx)
        return self._pY(qF, E), qF, pF

    def expected_loglik(self, X, y, idx=None, E=None, **kwargs):
        """Fused form of ``forward``'s ``pY.log_prob(y).mean(0).sum()``, exact: (value, qF, pF).  ``X`` is accepted for the
        signature of the spatial models and unused, ``E`` likewise.  The 3-tuple is ``PNMF``'s: ``train`` and
        ``train_batched`` unpack four values and therefore do not run an ``FA`` (nor a ``PNMF``); write the loop by hand."""
        _known_kwargs("FA", kwargs, ())
        qF, pF = self.prior() if idx is None else self.prior.forward_batched(idx)
        ll = gaussian_expected_loglik([qF], [self.W], self.b, _noise_sd(self.noise), y)
        return ll, qF, pF

    def score(self, X, y, idx=None, **kwargs):
        """``GaussianScore`` of ``y`` (D, B) for the fitted spots (or those of ``idx``); see ``RSF.score``.  The factors
        exist only for the fitted spots."""
        _known_kwargs("FA", kwargs, ())
        with torch.no_grad():
            qF = (self.prior() if idx is None else self.prior.forward_batched(idx))[0]
            return gaussian_score([qF], [self.W], self.b, _noise_sd(self.noise), y)

    def _residual_factors(self, X, idx, groupsX):
        """The factors exist only for the fitted spots (or those of ``idx``): ``X``, their coordinates, is used for the
        neighbour graph alone."""
        if groupsX is not None:
            raise TypeError("FA: groupsX= has no meaning here: the factors are per spot, not a GP's")
        qF = (self.prior() if idx is None else self.prior.forward_batched(idx))[0]
        B = X.shape[0] if idx is None else X[idx].shape[0]
        if qF.mean.shape[-1] != B:
            raise ValueError(f"FA: the factors exist only for the fitted spots ({qF.mean.shape[-1]} here), so {B} coordinates "
                             "cannot be scored; X is used for the neighbour graph alone")
        return qF
