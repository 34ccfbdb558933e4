"""Tensor-level entry points: torch CUDA tensors in, HIP kernels underneath.

PyTorch is used for storage, streams and (in ``parallel.py``) torch.distributed
only; every numeric step of the hot path runs in libgpzoo_hip.so.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import threading
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from ._lib import GPZ_F32, GPZ_F64, KernelDesc, SvgpProblem


@dataclass
class KernelSpec:
    """Flattened hyper-parameters of one gpzoo kernel object (see kernels.py)."""
    kind: int
    sigma: torch.Tensor            # (L,)
    lengthscale: torch.Tensor      # (L,)
    batched: bool                  # False: scalar parameters -> results drop the latent axis
    group_a: Optional[torch.Tensor] = None   # (L,) effective multiplier of r^2_group
    group_r2: Optional[torch.Tensor] = None  # (G,G)
    group_pow: float = 1.0

    @property
    def L(self) -> int:
        return int(self.sigma.numel())


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return GPZ_F32
    if t.dtype == torch.float64:
        return GPZ_F64
    raise TypeError(f"gpzoo_amd supports float32/float64 tensors, got {t.dtype}")


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("gpzoo_amd computes on the GPU only (HIP kernels, no CPU fallback): "
                               "move the model and inputs to a cuda device")


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device: torch.device):
    """torch's current stream ON THE TENSORS' DEVICE (not the process-wide current device)."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _same_device(*ts) -> torch.device:
    """All tensor arguments must be CUDA tensors of ONE device; returns it.  The library's launches,
    memsets and event records go to the current HIP device, so every entry point runs under
    ``torch.cuda.device(dev)`` with this device (a model moved with ``.to('cuda:1')`` while the process's
    current device is 0 would otherwise launch on GPU 0 against GPU-1 pointers)."""
    dev = None
    for t in ts:
        if t is None or not isinstance(t, torch.Tensor) or not t.is_floating_point():
            continue                       # integer group ids / index tables are moved by the wrappers
        if not t.is_cuda:
            raise RuntimeError("gpzoo_amd computes on the GPU only (HIP kernels, no CPU fallback): "
                               "move the model and inputs to a cuda device")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"gpzoo_amd: tensor arguments live on different devices ({dev} and {t.device})")
    if dev is None:
        raise RuntimeError("gpzoo_amd: no tensor argument to take the device from")
    return dev


def _on_device(fn):
    """Decorator: validate that every tensor argument shares one CUDA device and make it current for the call."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        flat = [a for a in args if isinstance(a, torch.Tensor)] + [v for v in kwargs.values() if isinstance(v, torch.Tensor)]
        for a in args:
            if isinstance(a, KernelSpec):
                flat += [a.sigma, a.lengthscale, a.group_a, a.group_r2]
        dev = _same_device(*flat)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return wrapped


_workspaces: dict = {}


def _workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    """Scratch buffer of at least ``nbytes`` for the library call about to be issued.  One buffer per
    (device, stream): calls on one stream are ordered and may share it, calls on different streams may not."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        _workspaces.pop(key, None)
        ws = None
        ws = torch.empty(int(nbytes * 1.05) + 4096, dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def release_workspaces():
    _workspaces.clear()


def _desc(spec: KernelSpec, dtype: torch.dtype, keep: list) -> KernelDesc:
    def prep(t):
        if t is None:
            return None
        t = t.detach().to(dtype).contiguous()
        keep.append(t)
        return t
    sig, ell = prep(spec.sigma.reshape(-1)), prep(spec.lengthscale.reshape(-1))
    ga, gr2 = prep(spec.group_a), prep(spec.group_r2)
    d = KernelDesc()
    d.kind, d.n_latent, d.dtype = spec.kind, spec.L, _dt(sig)
    d.n_groups = 0 if gr2 is None else int(gr2.shape[0])
    d.sigma, d.lengthscale = sig.data_ptr(), ell.data_ptr()
    d.group_a = None if ga is None else ga.data_ptr()
    d.group_r2 = None if gr2 is None else gr2.data_ptr()
    d.group_pow = float(spec.group_pow)
    return d


@_on_device
def kfill(spec: KernelSpec, A: torch.Tensor, B: torch.Tensor, gA=None, gB=None, jitter: float = 0.0,
          out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """K[l,i,j] = k_l(A_i, B_j): (L,nA,nB), or (nA,nB) for scalar-parameter kernels."""
    _need_cuda(A, B, spec.sigma)
    lib = _lib.load()
    keep: list = []
    A = A.detach().contiguous()
    B = B.detach().to(A.dtype).contiguous()
    if A.dim() != 2 or B.dim() != 2 or A.shape[1] != B.shape[1]:
        raise ValueError(f"expected (n,d) inputs with equal d, got {tuple(A.shape)} and {tuple(B.shape)}")
    d = _desc(spec, A.dtype, keep)
    if spec.kind == _lib.KERNEL_MGGP_RBF:
        gA, gB = _group_ids(gA, A.shape[0], A.device, "groupsX"), _group_ids(gB, B.shape[0], A.device, "groupsZ")
        G = int(spec.group_r2.shape[0])
        # stand-alone call: checked here with ONE device-to-host sync for both id vectors (the fused pass flags it on the
        # device and rides on the sync it needs anyway)
        bad = [((g_ < 0) | (g_ >= G)).any() for g_ in (gA, gB) if g_.numel()]
        if bad and bool(torch.stack(bad).any()):
            raise IndexError("index out of range in self: a group id is outside [0, n_groups)")
    else:
        gA = gB = None
    odt = A.dtype if out_dtype is None else out_dtype
    nA, nB = A.shape[0], B.shape[0]
    K = torch.empty((spec.L, nA, nB), dtype=odt, device=A.device)
    if nA == 0 or nB == 0:      # an empty point set gives an empty matrix, as torch.cdist does for the reference
        return K if spec.batched else K[0]
    rc = lib.gpz_kfill(C.byref(d), _ptr(A), nA, _ptr(B), nB, A.shape[1], _ptr(gA), _ptr(gB), _ptr(K), nB,
                       nA * nB, float(jitter), _dt(K), _stream(A.device))
    _lib.check(rc, "gpz_kfill")
    return K if spec.batched else K[0]


@_on_device
def kgrad(spec: KernelSpec, A: torch.Tensor, B: torch.Tensor, Kbar: torch.Tensor, gA=None, gB=None,
          want_points: bool = True):
    """Backward of ``kfill`` (gpz_kgrad): Kbar = dLoss/dK of shape (L,nA,nB) -> (grad_theta (L,3) fp64 =
    d/d(sigma, lengthscale, effective group multiplier), grad_A (nA,d) fp64 or None)."""
    lib = _lib.load()
    keep: list = []
    A = A.detach().contiguous()
    B = B.detach().to(A.dtype).contiguous()
    d = _desc(spec, A.dtype, keep)
    nA, nB, L = A.shape[0], B.shape[0], spec.L
    Kbar = Kbar.detach().to(A.dtype).reshape(L, nA, nB).contiguous()
    if spec.kind == _lib.KERNEL_MGGP_RBF:
        gA, gB = _group_ids(gA, nA, A.device, "groupsX"), _group_ids(gB, nB, A.device, "groupsZ")
    else:
        gA = gB = None
    gth = torch.empty((L, 4), dtype=torch.float64, device=A.device)
    gpt = torch.empty((nA, 4), dtype=torch.float64, device=A.device) if want_points else None
    if nA == 0 or nB == 0:      # nothing to contract
        return gth.zero_()[:, :3], (gpt.zero_()[:, :A.shape[1]] if want_points else None)
    nbytes = lib.gpz_kgrad_workspace_bytes(nA, L)
    ws = _workspace(A.device, nbytes)
    rc = lib.gpz_kgrad(C.byref(d), _ptr(A), nA, _ptr(B), nB, A.shape[1], _ptr(gA), _ptr(gB), _ptr(Kbar), nB, nA * nB,
                       _ptr(gth), _ptr(gpt), _ptr(ws), ws.numel(), _stream(A.device))
    _lib.check(rc, "gpz_kgrad")
    return gth[:, :3], (gpt[:, :A.shape[1]] if want_points else None)


def pairwise_distance(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """Euclidean distances (nA,nB) -- what RBF.forward(return_distance=True) hands back."""
    one = torch.ones(1, dtype=A.dtype, device=A.device)
    return kfill(KernelSpec(_lib.KERNEL_DISTANCE, one, one, False), A, B)


def _group_ids(g, n: int, dev, name: str) -> torch.Tensor:
    """int64 group ids on the device, one per point (reference kernels.py:99-100, 177-178, 209-210 index the
    embedding with them: a wrong length or an id outside [0, n_groups) raises there, and here)."""
    g = g.detach().to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    if g.numel() != n:
        raise IndexError(f"{name} has {g.numel()} entries for {n} points")
    return g


def _raise_info(info: torch.Tensor, what: str):
    """LAPACK convention: info > 0 = not positive-definite (order of the failing minor), info < 0 = an argument
    was illegal -- here: a group id outside [0, n_groups), flagged by the covariance fill on the device."""
    if bool((info == -7).any()):
        raise RuntimeError(f"{what}: a hand-off inside the one-launch factorisation timed out (info = -7); "
                           "set GPZ_FACTOR_PATH=launches to use the launch-per-step path")
    if bool((info < 0).any()):
        raise IndexError("index out of range in self: a group id (groupsX / groupsZ) is outside [0, n_groups)")
    _raise_not_pd(info, what)


def _raise_not_pd(info: torch.Tensor, what: str):
    bad = torch.nonzero(info)
    b = int(bad[0, 0])
    k = int(info[b])
    prefix = f"(Batch element {b}): " if info.numel() > 1 else ""
    raise torch.linalg.LinAlgError(
        f"{what}: {prefix}The factorization could not be completed because the input is not "
        f"positive-definite (the leading minor of order {k} is not positive-definite).")


class _DeferredInfo:
    """`info` words of the factorisations launched inside one ``deferred_info()`` block, still on the device."""

    def __init__(self):
        self.items = []          # (info tensor, what, cache committed on trust or None)
        self.flags = []          # (0-d bool tensor "arguments valid", callable that raises torch's own error)
        self.checked = False

    def add(self, info: torch.Tensor, what: str, cache=None):
        self.items.append((info, what, cache))
        self.checked = False

    def add_flag(self, ok: torch.Tensor, reraise):
        self.flags.append((ok, reraise))
        self.checked = False

    def any_bad(self) -> Optional[torch.Tensor]:
        """0-d bool device tensor: some registered info word is non-zero or some argument check failed (no sync)."""
        words = [i.reshape(-1) != 0 for i, _, _ in self.items] + [~f.reshape(1) for f, _ in self.flags]
        return torch.cat(words).any() if words else None

    def check(self, keep: bool = False):
        """ONE device-to-host sync for everything registered so far; raises what the eager check would have raised
        (torch.linalg.LinAlgError / IndexError / RuntimeError) for the first failing call, after invalidating every
        factor cache that was committed on trust.  ``keep``: the registrations stay (a captured graph writes the same
        tensors at every replay)."""
        items, flags = self.items, self.flags
        if not keep:
            self.items, self.flags = [], []
        self.checked = True
        if not items and not flags:
            return
        words = [i.reshape(-1) != 0 for i, _, _ in items] + [~f.reshape(1) for f, _ in flags]
        if not bool(torch.cat(words).any()):
            return
        for _, _, cache in items:
            if cache is not None:
                cache.invalidate()
        for info, what, _ in items:        # in call order: a failed factorisation comes before the NaN moments it produced
            if bool(info.any()):
                _raise_info(info, what)
        for ok, reraise in flags:
            if not bool(ok):
                reraise()


_deferred = threading.local()


@contextlib.contextmanager
def deferred_info():
    """Inside the block, forward passes do not stop the launch queue to read their factorisation's ``info`` word: it
    stays on the device and is read ONCE when the block ends (or at ``.check()`` on the yielded object), raising what
    the call itself would have raised -- torch.linalg.LinAlgError for a Kzz that is not positive-definite (gp.py:213,
    270, 360).  A training step wraps forward + ``loss.backward()`` in it and puts the optimiser step behind it: the
    backward pass's launches are queued while the forward still runs (at the notebooks' sizes the eager check costs a
    drained queue per step: 0.4 ms of a 4 ms step at BASELINE configs[1]), a failed factorisation still raises before
    the parameters are touched.  What the block computed from a failed factor is garbage, as it would be unreachable
    eagerly.  Nested blocks register with the innermost one."""
    d = _DeferredInfo()
    stack = _deferred.__dict__.setdefault("stack", [])
    stack.append(d)
    try:
        yield d
    except BaseException:
        stack.pop()
        raise
    stack.pop()
    d.check()


def _deferring():
    stack = _deferred.__dict__.get("stack")
    return stack[-1] if stack else None


def checked_dist(cls, *args, **kwargs):
    """``cls(*args, **kwargs)`` -- a torch distribution -- with its argument validation (a device reduction and a HOST
    SYNC per constrained argument: ``Normal(loc, scale)`` stops the launch queue twice) moved to the end of the enclosing
    ``deferred_info()`` block: the constraint checks are queued as device flags, read with the block's one sync, and a
    violation raises what the constructor itself raises (it is re-run with validation on).  Outside a block: the plain
    constructor."""
    d = _deferring()
    if d is None or kwargs.get("validate_args") is False:
        return cls(*args, **kwargs)
    from torch import distributions as _D
    if not _D.Distribution._validate_args:          # validation switched off globally: nothing to defer
        return cls(*args, **kwargs)
    dist = cls(*args, validate_args=False, **kwargs)
    oks = []
    for name, constraint in dist.arg_constraints.items():
        if getattr(constraint, "is_dependent", False) or name not in dist.__dict__:
            continue
        oks.append(constraint.check(getattr(dist, name)).all())
    if oks:
        d.add_flag(torch.stack(oks).all(), lambda: cls(*args, validate_args=True, **kwargs))
    return dist


def freeze_spec(spec: KernelSpec) -> KernelSpec:
    """The same kernel with private copies of its (tiny) tensors: what a backward pass must hold so that edits of the
    live parameters between forward and backward (``.data`` writes, optimiser steps of another closure) cannot change
    the problem it differentiates."""
    cp = lambda t: None if t is None else t.detach().contiguous().clone()
    return KernelSpec(spec.kind, cp(spec.sigma), cp(spec.lengthscale), spec.batched, cp(spec.group_a), cp(spec.group_r2),
                      spec.group_pow)


@_on_device
def cholesky(A: torch.Tensor) -> torch.Tensor:
    """Lower Cholesky factor of (M,M) or (L,M,M), fp32 or fp64 storage (fp64 arithmetic); raises
    torch.linalg.LinAlgError when a matrix is not positive-definite (what gp.py:213/270/360 callers see)."""
    _need_cuda(A)
    lib = _lib.load()
    M = A.shape[-1]
    W = A.detach().reshape(-1, M, M).contiguous().clone()
    batch = W.shape[0]
    info = torch.empty(batch, dtype=torch.int32, device=A.device)
    nbytes = lib.gpz_potrf_workspace_bytes(M, batch)
    ws = _workspace(A.device, nbytes)
    rc = lib.gpz_potrf_batched(_ptr(W), _dt(W), M, M, M * M, batch, _ptr(info), _ptr(ws), ws.numel(), _stream(A.device))
    _lib.check(rc, "gpz_potrf_batched")
    if bool(info.any()):
        _raise_info(info, "linalg.cholesky")
    return W.reshape(A.shape)


@_on_device
def solve_triangular_lower(Lc: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """Lc^{-1} B for lower-triangular (.., M, M) and (.., M, N): blocked forward substitution (gpz_trsm_lln_batched)."""
    _need_cuda(Lc, B)
    lib = _lib.load()
    M, N = B.shape[-2], B.shape[-1]
    Lw = Lc.detach().to(B.dtype).reshape(-1, M, M).contiguous()
    Bw = B.detach().reshape(-1, M, N).contiguous().clone()
    batch = Bw.shape[0]
    if Lw.shape[0] != batch:
        Lw = Lw.expand(batch, M, M).contiguous()
    nbytes = lib.gpz_trsm_workspace_bytes(M, N, batch)
    ws = _workspace(B.device, nbytes)
    rc = lib.gpz_trsm_lln_batched(_ptr(Lw), M, M * M, _ptr(Bw), N, M * N, _dt(Bw), M, N, batch, _ptr(ws), ws.numel(),
                                  _stream(B.device))
    _lib.check(rc, "gpz_trsm_lln_batched")
    return Bw.reshape(B.shape)


class FactorCache:
    """Device buffer for chol(Kzz), its inverse and log-determinant, reused while its inputs are unchanged.

    Validity is decided by CONTENT, not by tensor identity: next to the factor the cache keeps a byte copy
    of everything the factor depends on (Z, sigma, lengthscale, effective group multiplier, the group r^2
    table, groupsZ) and compares it on the device before every use (one concatenation + one ``torch.equal``,
    a few KB), plus a host key (kernel family, L, exponent, jitter, dtype, shapes).  In-place edits through
    ``.data`` (``p.data.fill_()``, ``p.data = ...``), re-created Parameters that land on a freed pointer and
    optimiser steps are therefore all seen (SURVEY §8f "next" #3: the reference refactors Kzz every step even
    when those are frozen)."""

    def __init__(self):
        self.buf = None
        self.key = None
        self.snap = None
        self._pending = None
        # Counts the factorisations written into ``buf`` (and its invalidations).  A forward pass notes the value it
        # committed; its backward pass may skip the content check only while the counter still has that value, i.e.
        # while no other call has refactored into the shared buffer in between.
        self.generation = 0
        # Counts the calls that wrote their q(U) operands (LuE^T, muE, un-whitened LuE) behind the factor -- every call
        # on the buffer but a backward that took them from it.  A backward pass may do that (factor_cache_valid = 3)
        # only while this is still the value its forward left.
        self.qu_generation = 0
        self._rebuilds = False

    @staticmethod
    def fingerprint(tensors) -> torch.Tensor:
        return torch.cat([t.reshape(-1).view(torch.uint8) for t in tensors if t is not None])

    def attach(self, lib, p: "SvgpProblem", key, device, deps, trust: bool = False, trust_qu: bool = False):
        """``trust``: the caller vouches that the buffer still holds the factor of exactly these ``deps`` -- the
        backward pass of the call whose forward committed it, holding private copies of the inputs and having checked
        that ``generation`` is still the value that forward saw -- so the content comparison (a device reduction and a
        host sync) is skipped.  ``trust_qu`` (with ``trust``): no other forward has written its q(U) operands into the
        buffer since, so the backward takes them from there too."""
        nbytes = lib.gpz_svgp_factor_cache_bytes(C.byref(p))
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self.key = self.snap = None
            self.generation += 1
        if trust and self.key == key and self.snap is not None:
            p.factor_cache = self.buf.data_ptr()
            p.factor_cache_valid = 3 if trust_qu else 1
            if not trust_qu:
                self.qu_generation += 1
            self._pending = (key, self.snap)
            self._rebuilds = False
            return True
        fp = self.fingerprint(deps)
        valid = (self.key == key and self.snap is not None and self.snap.shape == fp.shape
                 and bool(torch.equal(self.snap, fp)))
        p.factor_cache = self.buf.data_ptr()
        p.factor_cache_valid = int(valid)
        self.qu_generation += 1
        self._pending = (key, fp)
        self._rebuilds = not valid
        return valid

    def invalidate(self):
        self.key = self.snap = None
        self.generation += 1

    def commit(self):
        self.key, self.snap = self._pending
        if self._rebuilds:                 # the launch just wrote a new factor into the buffer
            self.generation += 1
            self._rebuilds = False


def factor_key(spec: "KernelSpec", Z, jitter, dtype) -> tuple:
    """Host half of the cache key; the tensor contents are compared on the device (FactorCache.attach)."""
    G = 0 if spec.group_r2 is None else int(spec.group_r2.shape[0])
    return (spec.kind, spec.L, float(spec.group_pow), float(jitter), str(dtype), tuple(Z.shape), G)


def _problem(spec: KernelSpec, X, Z, mu, Lu_raw, jitter, whitened, gX, gZ, clamp_min, keep: list, groups: bool = True):
    """Fill a gpz_svgp_problem from tensors (inputs only); returns (problem, (L, M, N, dtype, device, deps)) where
    ``deps`` are the prepared tensors chol(Kzz) depends on (what FactorCache fingerprints).  ``groups=False``: the entry
    takes no group ids (gpz_vnngp, which refuses a multi-group kind itself and says so)."""
    dt = X.dtype
    if X.dim() != 2 or Z.dim() != 2 or X.shape[1] != Z.shape[1]:
        raise ValueError(f"expected X (N,d) and Z (M,d) with equal d, got {tuple(X.shape)} and {tuple(Z.shape)}")
    X = X.detach().contiguous()
    Z = Z.detach().to(dt).contiguous()
    L = spec.L
    M, N, dim = Z.shape[0], X.shape[0], X.shape[1]
    if mu.numel() != L * M or Lu_raw.numel() != L * M * M:
        raise ValueError(f"mu / Lu of shapes {tuple(mu.shape)} / {tuple(Lu_raw.shape)} do not match L={L} latents "
                         f"and M={M} inducing points")
    mu = mu.detach().to(dt).reshape(L, M).contiguous()
    Lu_raw = Lu_raw.detach().to(dt).reshape(L, M, M).contiguous()
    dev = X.device
    p = SvgpProblem()
    n0 = len(keep)
    p.k = _desc(spec, dt, keep)
    deps = [Z] + keep[n0:]
    p.dtype, p.whitened, p.d = _dt(X), int(whitened), dim
    p.N, p.M = N, M
    p.X, p.Z, p.mu, p.Lu_raw = X.data_ptr(), Z.data_ptr(), mu.data_ptr(), Lu_raw.data_ptr()
    if groups and spec.kind == _lib.KERNEL_MGGP_RBF:
        if gX is None or gZ is None:
            raise ValueError("multi-group kernels need groupsX and groupsZ")
        gX, gZ = _group_ids(gX, N, dev, "groupsX"), _group_ids(gZ, M, dev, "groupsZ")
        p.gX, p.gZ = gX.data_ptr(), gZ.data_ptr()
        deps.append(gZ)
    p.jitter, p.var_clamp_min = float(jitter), float(clamp_min)
    keep.extend([X, Z, mu, Lu_raw, gX, gZ])
    return p, (L, M, N, dt, dev, deps)


@_on_device
def svgp_forward(spec: KernelSpec, X, Z, mu, Lu_raw, jitter: float, whitened: bool, *, gX=None, gZ=None,
                 y=None, noise_sd: Optional[float] = None, clamp_min: float = 1e-6, chunk: int = 0,
                 want_moments: bool = True, want_Lu: bool = True, want_chol: bool = False,
                 check_info: bool = True, cache: Optional[FactorCache] = None,
                 retain_wt: float = 0.0, materialize_kzx: Optional[bool] = None, narrow_tiles: bool = False,
                 panel_products: bool = False) -> dict:
    """One fused forward pass (gpz_svgp_forward).  Returns a dict with mean, scale
    (L,N), Lu (L,M,M), chol (L,M,M), kl (L,), loglik (L,), elbo () -- fp64 scalars.
    ``retain_wt`` > 0: keep Wt of every chunk for ``svgp_backward(wt_cache=out["wt_cache"])`` when it fits
    in that fraction of the free device memory (288 GB HBM: 52 GB at N=200k, M=2048, L=32, fp32).
    ``materialize_kzx``: True = write every Kzx chunk to HBM and run the triangular product on it (the reference's
    structure), False = the product that generates its covariance operand itself (fp32 RBF / Matern-1/2, -3/2, -5/2, d <= 2), None =
    the library's choice; ``narrow_tiles``: the 128 x 128-tile kernel of the other precisions for the two big fp32
    products; ``panel_products`` (fp32, M <= 512): both products in one launch on 64-column panels held in LDS.  Same Wt
    bits on every path."""
    _need_cuda(X, Z, mu, Lu_raw)
    if X.dim() == 2 and X.shape[0] == 0 and Z.dim() == 2 and Z.shape[0] > 0:
        # No data points: q(F) is empty and the ELBO is -sum(KL), as the reference's torch code gives for an (0,d) X.
        # The library wants N >= 1: evaluate at one stand-in point (the first inducing point) and drop its column.
        o = svgp_forward(spec, Z[:1].to(X.dtype), Z, mu, Lu_raw, jitter, whitened, gX=None if gZ is None else gZ[:1], gZ=gZ,
                         clamp_min=clamp_min, want_moments=want_moments, want_Lu=want_Lu, want_chol=want_chol,
                         check_info=check_info, cache=cache)
        for k in ("mean", "scale"):
            if k in o:
                o[k] = o[k][:, :0]
        o["loglik"] = torch.zeros_like(o["kl"])
        o["elbo"] = -o["kl"].sum()
        return o
    lib = _lib.load()
    keep: list = []
    p, (L, M, N, dt, dev, deps) = _problem(spec, X, Z, mu, Lu_raw, jitter, whitened, gX, gZ, clamp_min, keep)
    out = {}
    if materialize_kzx is not None:
        p.flags |= _lib.SVGP_MATERIALIZE_KZX if materialize_kzx else _lib.SVGP_GENERATE_KZX
    if narrow_tiles:
        p.flags |= _lib.SVGP_NARROW_TILES
    if panel_products:               # fp32, M <= 512: both products in one launch, panel by panel (csrc/gemmp.hip)
        p.flags |= _lib.SVGP_PANEL_PRODUCTS
    if y is not None:
        y = y.detach().to(dt).reshape(L, N).contiguous()
        p.y, p.noise_sd = y.data_ptr(), float(noise_sd)
    if want_moments:
        out["mean"] = torch.empty((L, N), dtype=dt, device=dev)
        out["scale"] = torch.empty((L, N), dtype=dt, device=dev)
        p.mean, p.scale = out["mean"].data_ptr(), out["scale"].data_ptr()
    if want_Lu:
        out["Lu"] = torch.empty((L, M, M), dtype=dt, device=dev)
        p.Lu = out["Lu"].data_ptr()
    if want_chol:
        out["chol"] = torch.empty((L, M, M), dtype=dt, device=dev)
        p.chol = out["chol"].data_ptr()
    scal = torch.empty(2 * L + 1, dtype=torch.float64, device=dev)     # every entry is written by the pass (reduce / elbo_sum kernels)
    info = torch.empty(L, dtype=torch.int32, device=dev)
    p.kl, p.loglik, p.elbo = scal.data_ptr(), scal.data_ptr() + 8 * L, scal.data_ptr() + 16 * L
    p.info = info.data_ptr()
    if cache is not None:
        cache.attach(lib, p, factor_key(spec, Z, jitter, dt), dev, deps)
        out["qu_generation"] = cache.qu_generation   # this call writes its q(U) operands behind the factor
    if retain_wt > 0:
        need = lib.gpz_svgp_wt_cache_bytes(C.byref(p), int(chunk))
        if 0 < need <= retain_wt * torch.cuda.mem_get_info(dev)[0]:
            out["wt_cache"] = torch.empty(need, dtype=torch.uint8, device=dev)
            p.wt_cache = out["wt_cache"].data_ptr()
    nbytes = lib.gpz_svgp_workspace_bytes(C.byref(p), int(chunk))
    if nbytes == 0:
        _lib.check(-1, "gpz_svgp_workspace_bytes")
    ws = _workspace(dev, nbytes)
    rc = lib.gpz_svgp_forward(C.byref(p), int(chunk), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, "gpz_svgp_forward")
    out["path"] = lib.gpz_svgp_forward_path(C.byref(p), int(chunk))    # bit 0: wide tiles, bit 1: generated Kzx, 4: panel kernel
    later = _deferring() if check_info else None
    if later is not None:
        # inside deferred_info(): no sync here; the cache is committed on trust and invalidated by the block's check
        # should the factorisation have failed
        later.add(info, "linalg.cholesky", cache)
        check_info = False
    bad = check_info and bool(info.any())       # one device-to-host sync, shared by the cache decision and the raise
    if cache is not None:
        # a factor that failed must not be reused; without the host check the cache stays uncommitted
        if later is not None:
            cache.commit()
        elif not check_info or bad:
            cache.invalidate()
        else:
            cache.commit()
        out["factor_generation"] = cache.generation
    if bad:
        _raise_info(info, "linalg.cholesky")
    out["kl"], out["loglik"], out["elbo"] = scal[:L], scal[L:2 * L], scal[2 * L]
    out["info"] = info
    return out


@_on_device
def svgp_backward(spec: KernelSpec, X, Z, mu, Lu_raw, jitter: float, whitened: bool, g_mean, g_scale, scale, *,
                  gX=None, gZ=None, clamp_min: float = 1e-6, chunk: int = 0, cache: Optional[FactorCache] = None,
                  kernel_grads: bool = False, g_chol=None, wt_cache=None, g_kl=None, trust_cache: bool = False,
                  trust_qu: bool = False, narrow_tiles: bool = False, form: Optional[str] = None):
    """dLoss/dmu (L,M) and dLoss/dLu_raw (L,M,M) (gpz_svgp_backward); with ``kernel_grads`` also
    dLoss/d(sigma, lengthscale, effective group parameter) (L,3) and dLoss/dZ (M,d), both fp64.
    ``wt_cache``: the buffer a forward pass on the same inputs and ``chunk`` returned under "wt_cache".
    ``g_kl`` (L,): upstream gradient of the forward's per-latent ``kl``; its own
    gradient is folded into the results.  ``form``: "algebra" / "classic" / None (the library's choice by N / M): the
    N-sized work as one weighted symmetric accumulation plus M x M products, or as the products autograd would run."""
    _need_cuda(X, Z, mu, Lu_raw, g_mean, g_scale)
    if X.dim() == 2 and X.shape[0] == 0 and Z.dim() == 2 and Z.shape[0] > 0:
        # empty X (see svgp_forward): one stand-in point with zero upstream gradients leaves the KL / factor terms
        zero = torch.zeros((spec.L, 1), dtype=X.dtype, device=X.device)
        return svgp_backward(spec, Z[:1].to(X.dtype), Z, mu, Lu_raw, jitter, whitened, zero, zero, torch.ones_like(zero),
                             gX=None if gZ is None else gZ[:1], gZ=gZ, clamp_min=clamp_min, cache=cache,
                             kernel_grads=kernel_grads, g_chol=g_chol, g_kl=g_kl, trust_cache=trust_cache)
    lib = _lib.load()
    keep: list = []
    p, (L, M, N, dt, dev, deps) = _problem(spec, X, Z, mu, Lu_raw, jitter, whitened, gX, gZ, clamp_min, keep)
    info = torch.empty(L, dtype=torch.int32, device=dev)
    p.info = info.data_ptr()
    if narrow_tiles:                 # the 128 x 128-tile kernel for the fp32 products (csrc/gemm.hip), as in round 2
        p.flags |= _lib.SVGP_NARROW_TILES
    if form is not None:
        p.flags |= {"algebra": _lib.SVGP_BACKWARD_ALGEBRA, "classic": _lib.SVGP_BACKWARD_CLASSIC}[form]
    g = _lib.SvgpGrads()
    gm = g_mean.detach().to(dt).reshape(L, N).contiguous()
    gs = g_scale.detach().to(dt).reshape(L, N).contiguous()
    sc = scale.detach().to(dt).reshape(L, N).contiguous()
    grad_mu = torch.empty((L, M), dtype=dt, device=dev)
    grad_Lu = torch.empty((L, M, M), dtype=dt, device=dev)
    g.g_mean, g.g_scale, g.scale = gm.data_ptr(), gs.data_ptr(), sc.data_ptr()
    g.grad_mu, g.grad_Lu_raw = grad_mu.data_ptr(), grad_Lu.data_ptr()
    if kernel_grads and g_chol is not None:
        gc = g_chol.detach().to(dt).reshape(L, M, M).contiguous()
        keep.append(gc)
        g.g_chol = gc.data_ptr()
    if kernel_grads:
        gth = torch.zeros((L, 4), dtype=torch.float64, device=dev)
        gz = torch.zeros((M, 4), dtype=torch.float64, device=dev)
        g.grad_theta, g.grad_Z = gth.data_ptr(), gz.data_ptr()
    if g_kl is not None:
        gk = g_kl.detach().to(device=dev, dtype=torch.float64).reshape(-1).expand(L).contiguous()
        keep.append(gk)
        g.g_kl = gk.data_ptr()
    if cache is not None:
        cache.attach(lib, p, factor_key(spec, Z, jitter, dt), dev, deps, trust=trust_cache, trust_qu=trust_cache and trust_qu)
    if wt_cache is not None:
        if wt_cache.numel() != lib.gpz_svgp_wt_cache_bytes(C.byref(p), int(chunk)):
            raise ValueError("wt_cache does not belong to this problem / chunking")
        p.wt_cache, p.wt_cache_valid = wt_cache.data_ptr(), 1
    nbytes = lib.gpz_svgp_backward_workspace_bytes(C.byref(p), int(chunk))
    if nbytes == 0:
        _lib.check(-1, "gpz_svgp_backward_workspace_bytes")
    ws = _workspace(dev, nbytes)
    rc = lib.gpz_svgp_backward(C.byref(p), C.byref(g), int(chunk), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, "gpz_svgp_backward")
    if cache is not None and not (p.factor_cache_valid & 1):
        # the backward refactored (cache miss): keep the result only if the factorisation succeeded
        if bool(info.any()):
            cache.invalidate()
        else:
            cache.commit()
    if kernel_grads:
        return grad_mu, grad_Lu, gth[:, :3], gz[:, :X.shape[1]]
    return grad_mu, grad_Lu


@_on_device
def wsvgp_precomputed(W, sigma, mu, Lu_raw) -> dict:
    """q(F) moments from a caller-supplied W (L,N,M) or (N,M): WSVGP.forward_precomputed."""
    _need_cuda(W, mu, Lu_raw)
    lib = _lib.load()
    dt = W.dtype
    M = W.shape[-1]
    W3 = W.detach().reshape(-1, W.shape[-2], M).contiguous()
    L, N = W3.shape[0], W3.shape[1]
    mu2 = mu.detach().to(dt).reshape(-1, M).expand(L, M).contiguous()
    Lu3 = Lu_raw.detach().to(dt).reshape(-1, M, M).expand(L, M, M).contiguous()
    sig = sigma.detach().to(dt).reshape(-1).expand(L).contiguous()
    out = {"mean": torch.empty((L, N), dtype=dt, device=W.device), "scale": torch.empty((L, N), dtype=dt, device=W.device),
           "Lu": torch.empty((L, M, M), dtype=dt, device=W.device)}
    nbytes = lib.gpz_wsvgp_precomputed_workspace_bytes(L, N, M, _dt(W3))
    ws = _workspace(W.device, nbytes)
    rc = lib.gpz_wsvgp_precomputed(_ptr(W3), _ptr(sig), _ptr(mu2), _ptr(Lu3), L, N, M, _dt(W3), _ptr(out["mean"]),
                                   _ptr(out["scale"]), _ptr(out["Lu"]), _ptr(ws), ws.numel(), _stream(W.device))
    _lib.check(rc, "gpz_wsvgp_precomputed")
    return out


@_on_device
def wsvgp_precomputed_backward(W, sigma, mu, Lu_raw, g_mean, g_scale, scale):
    """dLoss/d(mu (L,M), raw Lu (L,M,M), sigma (L,) fp64) of ``wsvgp_precomputed`` (gpz_wsvgp_precomputed_backward);
    W is a constant of the graph."""
    lib = _lib.load()
    dt = W.dtype
    M = W.shape[-1]
    W3 = W.detach().reshape(-1, W.shape[-2], M).contiguous()
    L, N = W3.shape[0], W3.shape[1]
    mu2 = mu.detach().to(dt).reshape(-1, M).expand(L, M).contiguous()
    Lu3 = Lu_raw.detach().to(dt).reshape(-1, M, M).expand(L, M, M).contiguous()
    sig = sigma.detach().to(dt).reshape(-1).expand(L).contiguous()
    gm = g_mean.detach().to(dt).reshape(L, N).contiguous()
    gs = g_scale.detach().to(dt).reshape(L, N).contiguous()
    sc = scale.detach().to(dt).reshape(L, N).contiguous()
    grad_mu = torch.empty((L, M), dtype=dt, device=W.device)
    grad_Lu = torch.empty((L, M, M), dtype=dt, device=W.device)
    grad_sig = torch.empty(L, dtype=torch.float64, device=W.device)
    nbytes = lib.gpz_wsvgp_precomputed_backward_workspace_bytes(L, N, M, _dt(W3))
    ws = _workspace(W.device, nbytes)
    rc = lib.gpz_wsvgp_precomputed_backward(_ptr(W3), _ptr(sig), _ptr(mu2), _ptr(Lu3), L, N, M, _dt(W3), _ptr(gm), _ptr(gs),
                                            _ptr(sc), _ptr(grad_mu), _ptr(grad_Lu), _ptr(grad_sig), _ptr(ws), ws.numel(),
                                            _stream(W.device))
    _lib.check(rc, "gpz_wsvgp_precomputed_backward")
    return grad_mu, grad_Lu, grad_sig


@_on_device
def knn(X, Z, K: int) -> torch.Tensor:
    """(N,K) int64 indices of the K nearest rows of Z per row of X, ties to the lower index."""
    _need_cuda(X, Z)
    lib = _lib.load()
    X = X.detach().contiguous()
    Z = Z.detach().to(X.dtype).contiguous()
    idx = torch.empty((X.shape[0], K), dtype=torch.int64, device=X.device)
    rc = lib.gpz_knn(_ptr(X), X.shape[0], _ptr(Z), Z.shape[0], X.shape[1], K, _dt(X), _ptr(idx), _stream(X.device))
    _lib.check(rc, "gpz_knn")
    return idx


def morton_order(X: torch.Tensor) -> torch.Tensor:
    """(N,) int64 permutation that sorts the rows of X (N,d), d <= 4, along a Z-order (Morton) curve, 16 bits per
    coordinate, ties in index order: the ``point_order`` of ``vnngp_backward`` -- points that share their nearest
    inducing points become neighbours in the pass's per-point records -- and the search order of ``spatial_knn``.
    The bits of all coordinates are interleaved in one broadcast per block of rows (a handful of launches, not one per
    bit and coordinate)."""
    Xd = X.detach().double()
    lo = Xd.min(dim=0).values
    span = (Xd.max(dim=0).values - lo).clamp_min(1e-300)
    d = X.shape[1]
    bit = torch.arange(16, device=X.device)
    shift = bit.unsqueeze(0) * d + torch.arange(d, device=X.device).unsqueeze(1)        # (d,16): bit b of coordinate k
    key = torch.empty(X.shape[0], dtype=torch.int64, device=X.device)
    for r0 in range(0, X.shape[0], 1 << 20):
        q = ((Xd[r0:r0 + (1 << 20)] - lo) / span * 65535.0).round().to(torch.int64)
        key[r0:r0 + (1 << 20)] = (((q.unsqueeze(-1) >> bit) & 1) << shift).sum(dim=(1, 2))   # distinct bits: sum == or
    return torch.argsort(key, stable=True)


@_on_device
def spatial_knn(X, k: int = 6) -> torch.Tensor:
    """(N,k) int64 self-kNN graph of the rows of X (N,d), d <= 4, fp32 or fp64 (gpz_spatial_knn): row i holds the k
    points nearest to point i, itself excluded, ascending by (fp64 squared distance, index) -- the directed graph of
    squidpy's ``spatial_neighbors(coord_type="generic", n_neighs=k)`` wherever no exact tie falls on the k-th distance.
    Exact; the points are searched in ``morton_order(X)``."""
    _need_cuda(X)
    lib = _lib.load()
    X = X.detach().contiguous()
    if X.dim() != 2:
        raise ValueError(f"spatial_knn: X must be (N, d), got shape {tuple(X.shape)}")
    N, d = X.shape
    nb = lib.gpz_spatial_knn_workspace_bytes(N, d, int(k))
    if nb == 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    order = morton_order(X)
    idx = torch.empty((N, int(k)), dtype=torch.int64, device=X.device)
    ws = _workspace(X.device, nb)
    rc = lib.gpz_spatial_knn(_ptr(X), N, d, int(k), _dt(X), _ptr(order), _ptr(idx), _ptr(ws), ws.numel(), _stream(X.device))
    _lib.check(rc, "gpz_spatial_knn")
    return idx


@_on_device
def morans_i(values, nbr) -> torch.Tensor:
    """(L,) fp64 Moran's I of every column of values (N,L), fp32 or fp64, over the neighbour table nbr (N,K) int64
    with row-normalised weights (gpz_morans_i; squidpy's ``spatial_autocorr(mode="moran")``).  A constant column gives
    NaN.  Sums in a fixed order: repeated calls agree bit for bit.  A table entry outside [0, N) or naming its own row
    raises ValueError (checked on the device; one synchronisation)."""
    _need_cuda(values)
    lib = _lib.load()
    V = values.detach().contiguous()
    if V.dim() != 2 or nbr.dim() != 2 or nbr.shape[0] != V.shape[0]:
        raise ValueError(f"morans_i: values (N, L) and nbr (N, K) expected, got {tuple(V.shape)} and {tuple(nbr.shape)}")
    nbr = nbr.to(device=V.device, dtype=torch.int64).contiguous()
    N, L = V.shape
    K = nbr.shape[1]
    nb = lib.gpz_morans_i_workspace_bytes(N, L, K)
    if nb == 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    out = torch.empty(L, dtype=torch.float64, device=V.device)
    info = torch.empty(1, dtype=torch.int32, device=V.device)
    ws = _workspace(V.device, nb)
    rc = lib.gpz_morans_i(_ptr(V), N, L, _dt(V), _ptr(nbr), K, _ptr(out), _ptr(info), _ptr(ws), ws.numel(),
                          _stream(V.device))
    _lib.check(rc, "gpz_morans_i")
    if int(info.item()) != 0:
        raise ValueError("morans_i: the neighbour table has an entry outside [0, N) or naming its own row")
    return out


@_on_device
def knn_mean(X, F, Z, K: int, return_index: bool = False):
    """(M,L) fp64 mean of F (N,L) over the K rows of X (N,d) nearest to each row of Z (M,d), d <= 4, L <= 256
    (gpz_knn_mean): sklearn's ``KNeighborsRegressor(n_neighbors=K).fit(X, F).predict(Z)``.  X and Z fp32 or fp64 (both
    are taken as fp64 when they differ), F fp32 or fp64.  The K smallest (fp64 squared distance, index) keys are selected exactly,
    ties to the lower index; sums in a fixed order: repeated calls agree bit for bit.  ``return_index``: also the
    (M,K) int64 table of the selected rows, each query's in ascending index order."""
    _need_cuda(X, F, Z)
    lib = _lib.load()
    if X.dim() != 2 or F.dim() != 2 or Z.dim() != 2:
        raise ValueError(f"knn_mean: X (N, d), F (N, L) and Z (M, d) expected, got {tuple(X.shape)}, {tuple(F.shape)} and "
                         f"{tuple(Z.shape)}")
    if F.shape[0] != X.shape[0]:
        raise ValueError(f"knn_mean: {X.shape[0]} rows of X but {F.shape[0]} of F")
    if Z.shape[1] != X.shape[1]:
        raise ValueError(f"knn_mean: X has {X.shape[1]} coordinates per point, Z {Z.shape[1]}")
    N, d = X.shape
    M, L, K = Z.shape[0], F.shape[1], int(K)
    if not 1 <= K <= N:
        raise ValueError(f"knn_mean: K={K} outside 1..N={N}")
    ct = X.dtype if X.dtype == Z.dtype else torch.float64       # (either cast is exact)
    X = X.detach().to(ct).contiguous()
    Z = Z.detach().to(ct).contiguous()
    F = F.detach().contiguous()
    nb = lib.gpz_knn_mean_workspace_bytes(N, M, d, K, L)
    if nb == 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    U = torch.empty((M, L), dtype=torch.float64, device=X.device)
    idx = torch.empty((M, K), dtype=torch.int64, device=X.device) if return_index else None
    ws = _workspace(X.device, nb)
    rc = lib.gpz_knn_mean(_ptr(X), N, _ptr(Z), M, d, _dt(X), _ptr(F), L, _dt(F), K, _ptr(U), _ptr(idx), _ptr(ws),
                          ws.numel(), _stream(X.device))
    _lib.check(rc, "gpz_knn_mean")
    return (U, idx) if return_index else U


def _kmeans_args(who: str, X, M: int):
    _need_cuda(X)
    if X.dim() != 2:
        raise ValueError(f"{who}: X must be (N, d), got shape {tuple(X.shape)}")
    _dt(X)
    return X.detach().contiguous(), X.shape[0], X.shape[1], int(M)


def _kmeans_centres(who: str, C, M: int, d: int, device):
    _need_cuda(C)
    if C.dtype != torch.float64 or tuple(C.shape) != (M, d) or not C.is_contiguous() or C.device != device:
        raise ValueError(f"{who}: C must be a contiguous ({M}, {d}) float64 tensor on {device}, got {tuple(C.shape)} "
                         f"{C.dtype} on {C.device}")


@_on_device
def kmeans_seed(X, M: int, u):
    """k-means++ seeding of M centres among the rows of X (N,d), d <= 4, fp32 or fp64, from the uniform draws u (M,T)
    fp64 (gpz_kmeans_seed; sklearn's ``_kmeans_plusplus`` with the random stream passed in, T = 2 + floor(ln M) trials per
    centre).  Returns ``(idx (M,) int64, C (M,d) fp64)``.  Sums in a fixed order: repeated calls agree bit for bit."""
    X, N, d, M = _kmeans_args("kmeans_seed", X, M)
    _need_cuda(u)
    if u.dim() != 2 or u.shape[0] != M or u.dtype != torch.float64:
        raise ValueError(f"kmeans_seed: u must be ({M}, T) float64, got {tuple(u.shape)} {u.dtype}")
    u = u.detach().to(X.device).contiguous()
    T = u.shape[1]
    lib = _lib.load()
    nb = lib.gpz_kmeans_seed_workspace_bytes(N, d, M, T)
    if nb == 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    idx = torch.empty(M, dtype=torch.int64, device=X.device)
    C = torch.empty((M, d), dtype=torch.float64, device=X.device)
    ws = _workspace(X.device, nb)
    rc = lib.gpz_kmeans_seed(_ptr(X), N, d, _dt(X), M, T, _ptr(u), _ptr(idx), _ptr(C), _ptr(ws), ws.numel(), _stream(X.device))
    _lib.check(rc, "gpz_kmeans_seed")
    return idx, C


def kmeans_state(device) -> torch.Tensor:
    """A zeroed gpz_kmeans_state record on ``device`` for ``kmeans_lloyd``: (4,) int64 -- iterations done, stop reason
    (0 none / 1 labels / 2 tol), the last shift (the bits of an fp64: ``state[2:3].view(torch.float64)``), points relocated."""
    return torch.zeros(4, dtype=torch.int64, device=device)


@_on_device
def kmeans_lloyd(X, C, labels, state, tol_abs: float, iters: int):
    """Enqueue up to ``iters`` further Lloyd iterations on the centres C (M,d) fp64, IN PLACE (gpz_kmeans_lloyd).  labels
    (N,) int32 in/out (-1 everywhere before the first iteration), state from ``kmeans_state``; every launch returns at
    once when the record holds a stop reason, so nothing here synchronises: read ``state`` once per block of
    iterations.  Returns None."""
    X, N, d, M = _kmeans_args("kmeans_lloyd", X, C.shape[0] if C.dim() == 2 else 0)
    _kmeans_centres("kmeans_lloyd", C, M, d, X.device)
    _need_cuda(labels, state)
    if labels.dtype != torch.int32 or tuple(labels.shape) != (N,) or not labels.is_contiguous():
        raise ValueError(f"kmeans_lloyd: labels must be a contiguous ({N},) int32 tensor, got {tuple(labels.shape)} {labels.dtype}")
    if state.dtype != torch.int64 or tuple(state.shape) != (4,) or not state.is_contiguous():
        raise ValueError("kmeans_lloyd: state must come from ops.kmeans_state")
    lib = _lib.load()
    nb = lib.gpz_kmeans_lloyd_workspace_bytes(N, d, M)
    if nb == 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    ws = _workspace(X.device, nb)
    rc = lib.gpz_kmeans_lloyd(_ptr(X), N, d, _dt(X), _ptr(C), M, float(tol_abs), int(iters), _ptr(labels), _ptr(state),
                              _ptr(ws), ws.numel(), _stream(X.device))
    _lib.check(rc, "gpz_kmeans_lloyd")


@_on_device
def kmeans_assign(X, C, labels=None, return_d2: bool = False):
    """The nearest centre of every row of X (N,d) among C (M,d) fp64, ties to the lower index (gpz_kmeans_assign).
    ``labels=None``: returns ``(labels (N,) int32, inertia)``; given labels (N,) int32 are kept and only their inertia is
    computed.  inertia is a 0-d fp64 tensor on the device; ``return_d2`` adds the (N,) fp64 squared distances."""
    X, N, d, M = _kmeans_args("kmeans_assign", X, C.shape[0] if C.dim() == 2 else 0)
    _kmeans_centres("kmeans_assign", C, M, d, X.device)
    keep = labels is not None
    if keep:
        _need_cuda(labels)
        if labels.dtype != torch.int32 or tuple(labels.shape) != (N,) or not labels.is_contiguous():
            raise ValueError(f"kmeans_assign: labels must be a contiguous ({N},) int32 tensor, got {tuple(labels.shape)} {labels.dtype}")
    else:
        labels = torch.full((N,), -1, dtype=torch.int32, device=X.device)
    lib = _lib.load()
    nb = lib.gpz_kmeans_assign_workspace_bytes(N, d, M)
    if nb == 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    d2 = torch.empty(N, dtype=torch.float64, device=X.device) if return_d2 else None
    inertia = torch.empty((), dtype=torch.float64, device=X.device)
    ws = _workspace(X.device, nb)
    rc = lib.gpz_kmeans_assign(_ptr(X), N, d, _dt(X), _ptr(C), M, int(keep), _ptr(labels), _ptr(d2), _ptr(inertia), _ptr(ws),
                               ws.numel(), _stream(X.device))
    _lib.check(rc, "gpz_kmeans_assign")
    return (labels, inertia, d2) if return_d2 else (labels, inertia)


def kernel_gram_plan(N: int, M: int, n_latent: int, dtype: torch.dtype) -> dict:
    """How ``kernel_gram`` covers a shape (gpz_kernel_gram_plan, a host-only query: no device needed): ``tile`` (rows and
    columns of an output tile), ``col_step`` (columns of X per step of a workgroup), ``n_splits`` and ``cols_per_split`` of
    the N-splits (the last one may be shorter), ``workspace_bytes(R)`` of the call with R right-hand sides per latent."""
    lib = _lib.load()
    code = GPZ_F32 if dtype == torch.float32 else GPZ_F64
    tile, step, splits, cols = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    rc = lib.gpz_kernel_gram_plan(int(N), int(M), int(n_latent), code, C.byref(tile), C.byref(step), C.byref(splits),
                                  C.byref(cols))
    if rc != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return dict(tile=tile.value, col_step=step.value, n_splits=splits.value, cols_per_split=cols.value,
                workspace_bytes=lambda R=1: int(lib.gpz_kernel_gram_workspace_bytes(int(N), int(M), int(n_latent), int(R), code)))


GRAM_MAX_R = 64     # right-hand sides per latent one gpz_kernel_gram call takes


@_on_device
def kernel_gram(spec: KernelSpec, Z: torch.Tensor, X: torch.Tensor, F: torch.Tensor, jitter: float = 0.0):
    """Normal equations of the kernel least-squares fit of F on the inducing points (gpz_kernel_gram): ``(G, b)`` fp64 with
    G (n, M, M) = K_zx K_xz + jitter I and b (n, R, M) = K_zx F^T, K_zx = k(Z, X), in one pass over X without a stored
    K_zx.  Z (M,d), X (N,d), F (L,N).  A per-latent kernel (``spec.batched``) pairs latent l with row l of F: n = L, R = 1;
    a scalar-parameter kernel has one Gram matrix for all rows: n = 1, R = L (more than 64 rows are served 64 at a time).
    fp32 Z, X and parameters generate and multiply the covariance entries in fp32 (the bits ``kfill`` writes) inside an
    N-split; the splits are added in fp64 in a fixed order: repeated calls agree bit for bit."""
    _need_cuda(Z, X, F, spec.sigma)
    lib = _lib.load()
    if Z.dim() != 2 or X.dim() != 2 or F.dim() != 2 or Z.shape[1] != X.shape[1] or F.shape[1] != X.shape[0]:
        raise ValueError(f"kernel_gram: Z (M, d), X (N, d) and F (L, N) expected, got {tuple(Z.shape)}, {tuple(X.shape)} and "
                         f"{tuple(F.shape)}")
    ct = torch.float32 if Z.dtype == X.dtype == spec.sigma.dtype == spec.lengthscale.dtype == torch.float32 else torch.float64
    Z = Z.detach().to(ct).contiguous()
    X = X.detach().to(ct).contiguous()
    F = F.detach().to(ct).contiguous()
    (M, d), N, L = Z.shape, X.shape[0], F.shape[0]
    if spec.batched and spec.L != L:
        raise ValueError(f"kernel_gram: the kernel has parameters for {spec.L} latents, F has {L} rows")
    n, R = (L, 1) if spec.batched else (1, L)
    keep: list = []
    desc = _desc(spec if spec.batched else KernelSpec(spec.kind, spec.sigma.reshape(-1)[:1], spec.lengthscale.reshape(-1)[:1], False),
                 ct, keep)
    G = torch.empty((n, M, M), dtype=torch.float64, device=Z.device)
    b = torch.empty((n, R, M), dtype=torch.float64, device=Z.device)
    for r0 in range(0, R, GRAM_MAX_R):
        r = min(GRAM_MAX_R, R - r0)
        nb = lib.gpz_kernel_gram_workspace_bytes(N, M, n, r, _dt(Z))
        if nb == 0:
            raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
        ws = _workspace(Z.device, nb)
        bpart = b if r == R else torch.empty((n, r, M), dtype=torch.float64, device=Z.device)
        rc = lib.gpz_kernel_gram(C.byref(desc), _ptr(Z), M, _ptr(X), N, d, _ptr(F[r0:r0 + r] if not spec.batched else F), r,
                                 float(jitter), _ptr(G), _ptr(bpart), _ptr(ws), ws.numel(), _stream(Z.device))
        _lib.check(rc, "gpz_kernel_gram")
        if bpart is not b:
            b[:, r0:r0 + r] = bpart
    return G, b


def _nmf_args(X, W, H, who: str):
    _need_cuda(X, W, H)
    if X.dim() != 2 or W.dim() != 2 or H.dim() != 2 or W.shape[0] != X.shape[0] or H.shape[1] != X.shape[1] or W.shape[1] != H.shape[0]:
        raise ValueError(f"{who}: X (N, D), W (N, L) and H (L, D) expected, got {tuple(X.shape)}, {tuple(W.shape)} and {tuple(H.shape)}")
    if not (X.dtype == W.dtype == H.dtype):
        raise TypeError(f"{who}: X, W and H must share one dtype, got {X.dtype}, {W.dtype} and {H.dtype}")
    lib = _lib.load()
    (N, D), L = X.shape, W.shape[1]
    nb = lib.gpz_nmf_kl_workspace_bytes(N, D, L, _dt(X))
    if nb == 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return lib, N, D, L, nb


def _nmf_divergence(lib, X, W, H, N, D, L, nb, out):
    ws = _workspace(X.device, nb)
    rc = lib.gpz_nmf_kl_divergence(_ptr(X), _ptr(W), _ptr(H), N, D, L, _dt(X), _ptr(out), _ptr(ws), ws.numel(),
                                   _stream(X.device))
    _lib.check(rc, "gpz_nmf_kl_divergence")
    return float(out.item())


@_on_device
def nmf_kl_divergence(X, W, H) -> float:
    """sklearn's ``_beta_divergence(X, W, H, 1, square_root=True)`` for dense X (N,D) >= 0, W (N,L), H (L,D) on the GPU,
    fp32 or fp64 (gpz_nmf_kl_divergence): W H is formed tile by tile and never stored, the sums run in fp64 in a fixed
    order.  One synchronisation (the scalar comes back to the host)."""
    X, W, H = X.detach().contiguous(), W.detach().contiguous(), H.detach().contiguous()
    lib, N, D, L, nb = _nmf_args(X, W, H, "nmf_kl_divergence")
    out = torch.empty(1, dtype=torch.float64, device=X.device)
    return _nmf_divergence(lib, X, W, H, N, D, L, nb, out)


@_on_device
def nmf_kl_mu(X, W0, H0, max_iter: int = 200, tol: float = 1e-4):
    """KL-divergence NMF by multiplicative updates from (W0, H0): sklearn's ``_fit_multiplicative_update`` with
    ``beta_loss='kullback-leibler'`` and no regularisation, on the GPU (gpz_nmf_kl_update: the N x D product and
    quotient are never stored).  X (N,D) >= 0 and finite, W0 (N,L), H0 (L,D), one dtype (fp32 or fp64), L <= 64.
    Returns ``(W, H, n_iter)``; W0 and H0 are copied, not modified.  The control flow is sklearn's: the divergence
    before the loop, then after every 10th iteration (one scalar read back each), stopping when
    ``(previous_error - error) / error_at_init < tol``; ``tol = 0`` runs exactly ``max_iter`` iterations with no
    read-back.  Sums in a fixed order: the same input gives the same bits."""
    X = X.detach().contiguous()
    W, H = W0.detach().clone().contiguous(), H0.detach().clone().contiguous()
    lib, N, D, L, nb = _nmf_args(X, W, H, "nmf_kl_mu")

    def update(k):
        ws = _workspace(X.device, nb)
        rc = lib.gpz_nmf_kl_update(_ptr(X), _ptr(W), _ptr(H), N, D, L, _dt(X), k, _ptr(ws), ws.numel(), _stream(X.device))
        _lib.check(rc, "gpz_nmf_kl_update")

    out = torch.empty(1, dtype=torch.float64, device=X.device)
    return W, H, _nmf_mu_loop(update, lambda: _nmf_divergence(lib, X, W, H, N, D, L, nb, out), int(max_iter), tol)


def _nmf_mu_loop(update, divergence, max_iter: int, tol: float) -> int:
    """sklearn's control flow around ``update(k)`` (k iterations in place) and ``divergence()`` (a float): the divergence
    before the loop and after every 10th iteration; ``tol = 0``: ``max_iter`` iterations and no read-back.  Returns n_iter."""
    if max_iter < 1:
        return 0
    if not tol > 0:
        update(max_iter)
        return max_iter
    error_at_init = previous = divergence()
    n_iter = 0
    while n_iter < max_iter:
        k = min(10, max_iter - n_iter)
        update(k)
        n_iter += k
        if n_iter % 10 == 0:
            error = divergence()
            if (previous - error) / error_at_init < tol:
                break
            previous = error
    return n_iter


def _whole_counts(counts, who: str):
    """The ``SparseCounts`` behind ``counts`` (itself or its ``.T``); views ``y[:, idx]`` are refused."""
    from .likelihoods import SparseCounts, TransposedCounts
    if isinstance(counts, TransposedCounts):
        counts = counts.T
    if not isinstance(counts, SparseCounts):
        raise TypeError(f"{who}: counts must be a SparseCounts or its .T, got {type(counts).__name__}")
    if counts.base is not counts:
        raise TypeError(f"{who}: counts is a view y[:, idx]; the whole SparseCounts is needed")
    return counts


def _count_ptrs(c):
    return [_ptr(getattr(c, k)) for k in c._PARTS]


def _nmf_sparse_args(counts, W, H, who: str):
    c = _whole_counts(counts, who)
    _need_cuda(W, H)
    if c.device != W.device:
        raise RuntimeError(f"gpzoo_amd: the counts live on {c.device}, the factors on {W.device}: move them with counts.to(device)")
    D, N = c.shape
    if W.dim() != 2 or H.dim() != 2 or W.shape[0] != N or H.shape[1] != D or W.shape[1] != H.shape[0]:
        raise ValueError(f"{who}: counts (D, N) with W (N, L) and H (L, D) expected, got {tuple(c.shape)}, {tuple(W.shape)} and "
                         f"{tuple(H.shape)}")
    if W.dtype != H.dtype:
        raise TypeError(f"{who}: W and H must share one dtype, got {W.dtype} and {H.dtype}")
    lib = _lib.load()
    L = W.shape[1]
    nb = lib.gpz_nmf_kl_sparse_workspace_bytes(N, D, c.nnz, L, _dt(W))
    if nb == 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return lib, c, N, D, L, nb


def _nmf_sparse_divergence(lib, c, W, H, N, D, L, nb, out):
    ws = _workspace(W.device, nb)
    rc = lib.gpz_nmf_kl_sparse_divergence(*_count_ptrs(c), _ptr(W), _ptr(H), N, D, c.nnz, L, _dt(W), _ptr(out), _ptr(ws),
                                          ws.numel(), _stream(W.device))
    _lib.check(rc, "gpz_nmf_kl_sparse_divergence")
    return float(out.item())


@_on_device
def nmf_kl_divergence_sparse(counts, W, H) -> float:
    """``nmf_kl_divergence`` of X (N, D) = counts^T for counts held as their non-zeros (gpz_nmf_kl_sparse_divergence):
    ``counts`` is a ``likelihoods.SparseCounts`` (D genes, N spots) or its ``.T``, W (N, L), H (L, D) fp32 or fp64 on the
    counts' device.  Summed in fp64 in a fixed order over the by-spot order."""
    W, H = W.detach().contiguous(), H.detach().contiguous()
    lib, c, N, D, L, nb = _nmf_sparse_args(counts, W, H, "nmf_kl_divergence_sparse")
    out = torch.empty(1, dtype=torch.float64, device=W.device)
    return _nmf_sparse_divergence(lib, c, W, H, N, D, L, nb, out)


@_on_device
def nmf_kl_mu_sparse(counts, W0, H0, max_iter: int = 200, tol: float = 1e-4):
    """``nmf_kl_mu`` of X (N, D) = counts^T over the stored non-zeros (gpz_nmf_kl_sparse_update): O(nnz L) per iteration,
    no N x D array anywhere.  ``counts``: a ``likelihoods.SparseCounts`` (D genes, N spots, not a view) or its ``.T``;
    W0 (N, L), H0 (L, D) on its device, one dtype (fp32 or fp64), L <= 64.  Returns ``(W, H, n_iter)``; W0 and H0 are
    copied.  Control flow, stopping rule and reproducibility are those of ``nmf_kl_mu``."""
    W, H = W0.detach().clone().contiguous(), H0.detach().clone().contiguous()
    lib, c, N, D, L, nb = _nmf_sparse_args(counts, W, H, "nmf_kl_mu_sparse")

    def update(k):
        ws = _workspace(W.device, nb)
        rc = lib.gpz_nmf_kl_sparse_update(*_count_ptrs(c), _ptr(W), _ptr(H), N, D, c.nnz, L, _dt(W), k, _ptr(ws), ws.numel(),
                                          _stream(W.device))
        _lib.check(rc, "gpz_nmf_kl_sparse_update")

    out = torch.empty(1, dtype=torch.float64, device=W.device)
    return W, H, _nmf_mu_loop(update, lambda: _nmf_sparse_divergence(lib, c, W, H, N, D, L, nb, out), int(max_iter), tol)


def nmf_kl_sparse_plan(N: int, D: int, L: int, nnz: int, dtype=torch.float32) -> dict:
    """How ``nmf_kl_mu_sparse`` covers a shape (gpz_nmf_kl_sparse_plan, a host-only query: no device needed):
    ``spot_chunk`` and ``gene_chunk`` (non-zeros of a spot's / a gene's row per wave; 0: rows are not split),
    ``n_gene_chunks`` (upper bound of the gene pass's work list), ``factors_padded`` (L rounded up to the kernel instance),
    ``colsum_rows`` (rows per block of the partial sums behind colsum(W) and rowsum(H)), ``workspace_bytes``."""
    lib = _lib.load()
    dt = GPZ_F32 if dtype == torch.float32 else GPZ_F64 if dtype == torch.float64 else -1
    sc, gc, fp, cr, nch = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    rc = lib.gpz_nmf_kl_sparse_plan(int(N), int(D), int(nnz), int(L), dt, C.byref(sc), C.byref(gc), C.byref(nch), C.byref(fp),
                                    C.byref(cr))
    if rc != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return dict(spot_chunk=sc.value, gene_chunk=gc.value, n_gene_chunks=nch.value, factors_padded=fp.value,
                colsum_rows=cr.value,
                workspace_bytes=int(lib.gpz_nmf_kl_sparse_workspace_bytes(int(N), int(D), int(nnz), int(L), dt)))


@_on_device
def counts_matmul(counts, Q, transpose: bool = False):
    """``X @ Q`` (N, k) for Q (D, k), or with ``transpose`` ``X.T @ Q`` (D, k) for Q (N, k), X (N, D) = counts^T held as its
    non-zeros (gpz_counts_matmul): fp64, k <= 128, every sum in a fixed order.  ``counts``: a ``SparseCounts`` or its ``.T``."""
    c = _whole_counts(counts, "counts_matmul")
    _need_cuda(Q)
    if c.device != Q.device:
        raise RuntimeError(f"gpzoo_amd: the counts live on {c.device}, Q on {Q.device}: move them with counts.to(device)")
    D, N = c.shape
    Q = Q.detach().to(torch.float64).contiguous()
    if Q.dim() != 2 or Q.shape[0] != (N if transpose else D):
        raise ValueError(f"counts_matmul: Q ({N if transpose else D}, k) expected, got {tuple(Q.shape)}")
    k = Q.shape[1]
    lib = _lib.load()
    nb = lib.gpz_counts_matmul_workspace_bytes(N, D, c.nnz, k, int(bool(transpose)))
    if nb == 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    out = torch.empty((D if transpose else N, k), dtype=torch.float64, device=Q.device)
    ws = _workspace(Q.device, nb)
    rc = lib.gpz_counts_matmul(*_count_ptrs(c), _ptr(Q), _ptr(out), N, D, c.nnz, k, int(bool(transpose)), _ptr(ws), ws.numel(),
                               _stream(Q.device))
    _lib.check(rc, "gpz_counts_matmul")
    return out


@_on_device
def vnngp_forward(spec: KernelSpec, X, Z, mu, Lu_raw, jitter: float, K: int, clamp_min: float = 5e-2,
                  check_info: bool = True, idx=None, keep_state: bool = False) -> dict:
    """VNNGP forward (gpz_vnngp_forward; RBF and Matern-1/2, -3/2, -5/2 specs): mean, scale (L,N), Lu, chol (L,M,M), idx
    (N,K).  ``keep_state``: also
    "state", the buffer ``vnngp_backward(state=...)`` of the same call takes the factor, S and the KL operands from."""
    _need_cuda(X, Z, mu, Lu_raw)
    lib = _lib.load()
    keep: list = []
    p, (L, M, N, dt, dev, deps) = _problem(spec, X, Z, mu, Lu_raw, jitter, False, None, None, clamp_min, keep, groups=False)
    out = {"mean": torch.empty((L, N), dtype=dt, device=dev), "scale": torch.empty((L, N), dtype=dt, device=dev),
           "Lu": torch.empty((L, M, M), dtype=dt, device=dev), "chol": torch.empty((L, M, M), dtype=dt, device=dev)}
    info = torch.empty(L, dtype=torch.int32, device=dev)
    p.mean, p.scale, p.Lu, p.chol = (out[k].data_ptr() for k in ("mean", "scale", "Lu", "chol"))
    p.info = info.data_ptr()
    out["kl"] = torch.empty(L, dtype=torch.float64, device=dev)      # KL(qU || pU) per latent
    p.kl = out["kl"].data_ptr()
    out["idx"] = knn(X, Z, K) if idx is None else idx
    if keep_state:
        out["state"] = torch.empty(lib.gpz_vnngp_state_bytes(C.byref(p)), dtype=torch.uint8, device=dev)
        p.factor_cache, p.factor_cache_valid = out["state"].data_ptr(), 0
    nbytes = lib.gpz_vnngp_workspace_bytes(C.byref(p), K)
    if nbytes == 0:
        _lib.check(-1, "gpz_vnngp_workspace_bytes")
    ws = _workspace(dev, nbytes)
    rc = lib.gpz_vnngp_forward(C.byref(p), K, _ptr(out["idx"]), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, "gpz_vnngp_forward")
    later = _deferring() if check_info else None
    if later is not None:
        later.add(info, "linalg.cholesky")
    elif check_info and bool(info.any()):
        _raise_info(info, "linalg.cholesky")
    return out


@_on_device
def vnngp_backward(spec: KernelSpec, X, Z, mu, Lu_raw, jitter: float, K: int, idx, g_mean, g_scale, *,
                   clamp_min: float = 5e-2, kernel_grads: bool = False, g_chol=None, g_kl=None, state=None,
                   point_order=None):
    """dLoss/dmu (L,M), dLoss/dLu_raw (L,M,M) of VNNGP (gpz_vnngp_backward); with ``kernel_grads`` also
    dLoss/d(sigma, lengthscale) (L,2) and dLoss/dZ (M,d), both fp64.  ``state``: what ``vnngp_forward(keep_state=True)``
    of the SAME inputs returned (consumed: good for one backward pass).  ``point_order`` (N,) int64: a permutation of
    the points the pass lays its records out in (``morton_order(X)``: the gather then reads runs of neighbouring records)."""
    _need_cuda(X, Z, mu, Lu_raw, g_mean, g_scale, idx)
    lib = _lib.load()
    keep: list = []
    p, (L, M, N, dt, dev, deps) = _problem(spec, X, Z, mu, Lu_raw, jitter, False, None, None, clamp_min, keep, groups=False)
    info = torch.empty(L, dtype=torch.int32, device=dev)
    p.info = info.data_ptr()
    g = _lib.SvgpGrads()
    gm = g_mean.detach().to(dt).reshape(L, N).contiguous()
    gs = g_scale.detach().to(dt).reshape(L, N).contiguous()
    grad_mu = torch.empty((L, M), dtype=dt, device=dev)
    grad_Lu = torch.empty((L, M, M), dtype=dt, device=dev)
    g.g_mean, g.g_scale = gm.data_ptr(), gs.data_ptr()
    g.grad_mu, g.grad_Lu_raw = grad_mu.data_ptr(), grad_Lu.data_ptr()
    if kernel_grads and g_chol is not None:
        gc = g_chol.detach().to(dt).reshape(L, M, M).contiguous()
        keep.append(gc)
        g.g_chol = gc.data_ptr()
    if kernel_grads:
        gth = torch.zeros((L, 4), dtype=torch.float64, device=dev)
        gz = torch.zeros((M, 4), dtype=torch.float64, device=dev)
        g.grad_theta, g.grad_Z = gth.data_ptr(), gz.data_ptr()
    if g_kl is not None:
        gk = g_kl.detach().to(device=dev, dtype=torch.float64).reshape(-1).expand(L).contiguous()
        keep.append(gk)
        g.g_kl = gk.data_ptr()
    idx = idx.contiguous()
    if point_order is not None:
        po = point_order.detach().to(device=dev, dtype=torch.int64).contiguous()
        if po.numel() != N:
            raise ValueError(f"point_order has {po.numel()} entries for {N} points")
        keep.append(po)
        g.point_order = po.data_ptr()
    if state is not None:
        if state.numel() != lib.gpz_vnngp_state_bytes(C.byref(p)):
            raise ValueError("state does not belong to this problem")
        p.factor_cache, p.factor_cache_valid = state.data_ptr(), 5
    nbytes = lib.gpz_vnngp_backward_workspace_bytes(C.byref(p), K)
    if nbytes == 0:
        _lib.check(-1, "gpz_vnngp_backward_workspace_bytes")
    ws = _workspace(dev, nbytes)
    rc = lib.gpz_vnngp_backward(C.byref(p), C.byref(g), K, _ptr(idx), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, "gpz_vnngp_backward")
    if kernel_grads:
        return grad_mu, grad_Lu, gth[:, :2], gz[:, :X.shape[1]]
    return grad_mu, grad_Lu


@_on_device
def poisson_nsf(mean, scale, eps, W_pos, V_pos, y, with_lgamma: bool = True):
    """Fused Monte-Carlo Poisson log-likelihood of the NSF models and its gradients (gpz_poisson_nsf).

    mean, scale (Lt,N); eps (E,Lt,N); W_pos (D,Lt) and V_pos (N,) positive; y (D,N).  Returns
    (loglik fp64 scalar, dmean, dscale, dW, dV) with the mean over the E samples already applied.
    Up to 32 samples go through one call (y is read once per pass whatever E is); more are split."""
    _need_cuda(mean, scale, eps, W_pos, V_pos, y)
    lib = _lib.load()
    f32 = torch.float32
    mean, scale = mean.detach().to(f32).contiguous(), scale.detach().to(f32).contiguous()
    eps, y = eps.detach().to(f32).contiguous(), y.detach().to(f32).contiguous()
    W_pos, V_pos = W_pos.detach().to(f32).contiguous(), V_pos.detach().to(f32).contiguous()
    # the entry wants 16-byte aligned arrays (include/gpzoo_hip.h); a contiguous view keeps its storage offset
    mean, scale, eps, W_pos, V_pos, y = (t if t.data_ptr() % 16 == 0 else t.clone()
                                         for t in (mean, scale, eps, W_pos, V_pos, y))
    Lt, N = mean.shape
    E, D = eps.shape[0], y.shape[0]
    dev = mean.device
    eg = 32                                  # samples per call (PMAXE of csrc/poisson.hip)
    total = torch.zeros((), dtype=torch.float64, device=dev)
    acc = [torch.zeros((Lt, N), dtype=f32, device=dev), torch.zeros((Lt, N), dtype=f32, device=dev),
           torch.zeros((D, Lt), dtype=f32, device=dev), torch.zeros((N,), dtype=f32, device=dev)]
    for e0 in range(0, E, eg):
        ee = min(eg, E - e0)
        ll = torch.empty(2, dtype=torch.float64, device=dev)
        out = [torch.empty_like(t) for t in acc]
        nbytes = lib.gpz_poisson_nsf_workspace_bytes(N, D, Lt, ee)
        ws = _workspace(dev, nbytes)
        rc = lib.gpz_poisson_nsf(_ptr(mean), _ptr(scale), _ptr(eps[e0:e0 + ee]), _ptr(W_pos), _ptr(V_pos), _ptr(y), N, D,
                                 Lt, ee, int(with_lgamma and e0 == 0), _ptr(ll), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                 _ptr(out[3]), _ptr(ws), ws.numel(), _stream(dev))
        _lib.check(rc, "gpz_poisson_nsf")
        wgt = ee / E
        total += wgt * ll[0]
        if with_lgamma and e0 == 0:
            total -= ll[1]          # the parameter-free lgamma(y+1) term is evaluated once
        for a_, o_ in zip(acc, out):
            a_.add_(o_, alpha=wgt)
    return (total, *acc)


def nb_nsf_plan(N: int, D: int, Lt: int, E: int) -> dict:
    """How ``nb_nsf`` covers a shape (gpz_nb_nsf_plan, a host-only query: no device needed): ``factors_padded`` (Lt rounded
    up to the kernel instance), ``aligned_rows`` (N % 4 == 0: rows of y move 16 bytes at a time), ``gene_slices`` and
    ``spot_slices`` (partial slabs of the spot pass and of the gene pass), ``workspace_bytes``."""
    lib = _lib.load()
    fp, al, gsl, ssl = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    rc = lib.gpz_nb_nsf_plan(int(N), int(D), int(Lt), int(E), C.byref(fp), C.byref(al), C.byref(gsl), C.byref(ssl))
    if rc != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return dict(factors_padded=fp.value, aligned_rows=bool(al.value), gene_slices=gsl.value, spot_slices=ssl.value,
                workspace_bytes=int(lib.gpz_nb_nsf_workspace_bytes(int(N), int(D), int(Lt), int(E))))


@_on_device
def nb_nsf(mean, scale, eps, W_pos, V_pos, theta_pos, y, with_lgamma: bool = True):
    """Fused Monte-Carlo negative-binomial log-likelihood of the NSF models and its gradients (gpz_nb_nsf): the step of
    ``poisson_nsf`` for pY = NegativeBinomial(total_count=theta[:, None], logits=log(rate) - log(theta[:, None])).

    mean, scale (Lt,N); eps (E,Lt,N); W_pos (D,Lt), V_pos (N,) and theta_pos (D,) positive; y (D,N) dense.  Returns
    (loglik fp64 scalar, dmean, dscale, dW, dV, dtheta) with the mean over the E samples already applied.
    Up to 32 samples go through one call; more are split, each part weighted by its share of the samples (the terms
    that do not depend on the sample then count once).  Nothing here waits for the device: the call can be captured in
    a graph.  A ``SparseCounts`` raises TypeError: -theta log1p(mu / theta) does not vanish where y = 0, so the step has
    no O(nnz) form."""
    from .likelihoods import SparseCounts
    if isinstance(y, SparseCounts):
        raise TypeError("nb_nsf: the negative-binomial step takes dense counts (its zero-count term depends on the rate, "
                        "so there is no sum over the non-zeros): pass y.to_dense()")
    _need_cuda(mean, scale, eps, W_pos, V_pos, theta_pos, y)
    lib = _lib.load()
    f32 = torch.float32
    mean, scale, eps, W_pos, V_pos, theta_pos, y = (t.detach().to(f32).contiguous()
                                                    for t in (mean, scale, eps, W_pos, V_pos, theta_pos, y))
    # the entry wants 16-byte aligned arrays (include/gpzoo_hip.h); a contiguous view keeps its storage offset
    mean, scale, eps, W_pos, V_pos, theta_pos, y = (t if t.data_ptr() % 16 == 0 else t.clone()
                                                    for t in (mean, scale, eps, W_pos, V_pos, theta_pos, y))
    Lt, N = mean.shape
    E, D = eps.shape[0], y.shape[0]
    if scale.shape != (Lt, N) or eps.shape != (E, Lt, N) or W_pos.shape != (D, Lt) or V_pos.shape != (N,) or \
            theta_pos.shape != (D,) or y.shape != (D, N):
        raise ValueError(f"nb_nsf: y {tuple(y.shape)}, mean {tuple(mean.shape)}, scale {tuple(scale.shape)}, eps "
                         f"{tuple(eps.shape)}, W {tuple(W_pos.shape)}, V {tuple(V_pos.shape)}, theta {tuple(theta_pos.shape)} "
                         "do not fit together")
    dev = mean.device
    eg = 32                                  # samples per call (NMAXE of csrc/nb.hip)
    total = torch.zeros((), dtype=torch.float64, device=dev)
    acc = [torch.zeros((Lt, N), dtype=f32, device=dev), torch.zeros((Lt, N), dtype=f32, device=dev),
           torch.zeros((D, Lt), dtype=f32, device=dev), torch.zeros((N,), dtype=f32, device=dev),
           torch.zeros((D,), dtype=f32, device=dev)]
    for e0 in range(0, E, eg):
        ee = min(eg, E - e0)
        ll = torch.empty(2, dtype=torch.float64, device=dev)
        out = [torch.empty_like(t) for t in acc]
        nbytes = lib.gpz_nb_nsf_workspace_bytes(N, D, Lt, ee)
        if nbytes == 0:
            raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
        ws = _workspace(dev, nbytes)
        rc = lib.gpz_nb_nsf(_ptr(mean), _ptr(scale), _ptr(eps[e0:e0 + ee]), _ptr(W_pos), _ptr(V_pos), _ptr(theta_pos),
                            _ptr(y), N, D, Lt, ee, int(with_lgamma and e0 == 0), _ptr(ll), _ptr(out[0]), _ptr(out[1]),
                            _ptr(out[2]), _ptr(out[3]), _ptr(out[4]), _ptr(ws), ws.numel(), _stream(dev))
        _lib.check(rc, "gpz_nb_nsf")
        wgt = ee / E
        # loglik[0] and dtheta carry the sample-independent terms in full in every part: the weights sum to one
        total += wgt * ll[0]
        if with_lgamma and e0 == 0:
            total -= ll[1]          # the parameter-free lgamma(y+1) term is evaluated once
        for a_, o_ in zip(acc, out):
            a_.add_(o_, alpha=wgt)
    return (total, *acc)


def gaussian_fa_plan(N: int, D: int, Lt: int) -> dict:
    """How ``gaussian_fa`` covers a shape (gpz_gaussian_fa_plan, a host-only query: no device needed): ``factors_padded``
    (Lt rounded up to the kernel instance), ``aligned_rows`` (N % 4 == 0: rows of y move 16 bytes at a time),
    ``gene_slices`` and ``spot_slices`` (partial slabs of the spot pass and of the gene pass), ``partials_bytes``."""
    lib = _lib.load()
    fp, al, gsl, ssl, nb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    rc = lib.gpz_gaussian_fa_plan(int(N), int(D), int(Lt), C.byref(fp), C.byref(al), C.byref(gsl), C.byref(ssl), C.byref(nb))
    if rc != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return dict(factors_padded=fp.value, aligned_rows=bool(al.value), gene_slices=gsl.value, spot_slices=ssl.value,
                partials_bytes=int(nb.value))


def gaussian_fa(mean, scale, W, b, noise_sd, y, grads: bool = True):
    """Fused exact expected Gaussian log-likelihood of the real-valued factor models and its gradients (gpz_gaussian_fa):
    E_q[sum log Normal(y | b[:, None] + W F, noise_sd[:, None])] under q(F) = Normal(mean, scale), in closed form -- no
    samples.

    mean, scale (Lt,N); W (D,Lt) real; b (D,); noise_sd (D,) positive standard deviations; y (D,N) dense.  Returns
    (loglik fp64 scalar, sse_per_gene fp64 (D,), dmean, dscale, dW, db, dnoise_sd), or the first two with
    ``grads=False`` (one pass over y instead of two).  ``sse_per_gene`` is the squared error of the predictive mean
    b + W mean; ``loglik`` also carries the variance of q(F).  Nothing here waits for the device: the call can be captured
    in a graph.  A ``SparseCounts`` raises TypeError: normalised data is dense.  So does a ``SparseExpression`` (centred
    log-normalised counts held as their non-zeros): that form goes through ``gaussian_fa_sparse``."""
    from .likelihoods import SparseCounts, SparseExpression
    if isinstance(y, SparseExpression):
        raise TypeError("gaussian_fa: takes a dense array; a SparseExpression goes through gaussian_fa_sparse")
    if isinstance(y, SparseCounts):
        raise TypeError("gaussian_fa: the Gaussian step takes dense real-valued data (normalised expression is dense): "
                        "a SparseCounts holds counts, pass the normalised array")
    return _gaussian_fa(mean, scale, W, b, noise_sd, y, grads)


@_on_device
def _gaussian_fa(mean, scale, W, b, noise_sd, y, grads):
    _need_cuda(mean, scale, W, b, noise_sd, y)
    lib = _lib.load()
    f32 = torch.float32
    mean, scale, W, b, noise_sd, y = (t.detach().to(f32).contiguous() for t in (mean, scale, W, b, noise_sd, y))
    # the entry wants 16-byte aligned arrays (include/gpzoo_hip.h); a contiguous view keeps its storage offset
    mean, scale, W, b, noise_sd, y = (t if t.data_ptr() % 16 == 0 else t.clone() for t in (mean, scale, W, b, noise_sd, y))
    if mean.dim() != 2 or y.dim() != 2:
        raise ValueError(f"gaussian_fa: mean {tuple(mean.shape)} must be (Lt, N) and y {tuple(y.shape)} (D, N)")
    Lt, N = mean.shape
    D = y.shape[0]
    if scale.shape != (Lt, N) or W.shape != (D, Lt) or b.shape != (D,) or noise_sd.shape != (D,) or y.shape != (D, N):
        raise ValueError(f"gaussian_fa: y {tuple(y.shape)}, mean {tuple(mean.shape)}, scale {tuple(scale.shape)}, W "
                         f"{tuple(W.shape)}, b {tuple(b.shape)}, noise_sd {tuple(noise_sd.shape)} do not fit together")
    dev = mean.device
    nb = C.c_int64()
    if lib.gpz_gaussian_fa_plan(N, D, Lt, None, None, None, None, C.byref(nb)) != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    ll = torch.empty(1, dtype=torch.float64, device=dev)
    sse = torch.empty(D, dtype=torch.float64, device=dev)
    out = [torch.empty((Lt, N), dtype=f32, device=dev), torch.empty((Lt, N), dtype=f32, device=dev),
           torch.empty((D, Lt), dtype=f32, device=dev), torch.empty((D,), dtype=f32, device=dev),
           torch.empty((D,), dtype=f32, device=dev)] if grads else [None] * 5
    ws = _workspace(dev, nb.value)
    rc = lib.gpz_gaussian_fa(_ptr(mean), _ptr(scale), _ptr(W), _ptr(b), _ptr(noise_sd), _ptr(y), N, D, Lt, _ptr(ll), _ptr(sse),
                             *(_ptr(t) for t in out), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, "gpz_gaussian_fa")
    return (ll[0], sse, *out) if grads else (ll[0], sse)


def gaussian_fa_sparse_plan(N: int, B: int, D: int, Lt: int, nnz: int) -> dict:
    """How ``gaussian_fa_sparse`` covers a shape (gpz_gaussian_fa_sparse_plan, a host-only query: no device needed):
    ``gene_chunk`` (stored entries of a gene row per wave of the gene pass), ``n_gene_chunks`` (the bound on the length of its
    work list), ``factors_padded`` (Lt rounded up to the kernel instance), ``workspace_bytes``."""
    lib = _lib.load()
    gc, fp, nch, nb = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    rc = lib.gpz_gaussian_fa_sparse_plan(int(N), int(B), int(D), int(Lt), int(nnz), C.byref(gc), C.byref(nch), C.byref(fp),
                                         C.byref(nb))
    if rc != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return dict(gene_chunk=gc.value, n_gene_chunks=nch.value, factors_padded=fp.value, workspace_bytes=int(nb.value))


def gaussian_fa_sparse(mean, scale, W, b, noise_sd, expr, idx=None, grads: bool = True):
    """``gaussian_fa`` for expression held as its stored entries minus a per-gene offset (gpz_gaussian_fa_sparse): exact sums
    over the non-zeros plus Lt x Lt Gram matrices -- O(nnz_B Lt + (B + D) Lt^2) work, nothing of D x B elements.

    expr: a ``likelihoods.SparseExpression`` (D, N), or the view ``expr[:, idx]`` of one.  mean, scale (Lt,B) with B = N, or
    B = len(idx) for a view; W (D,Lt) real; b, noise_sd (D,).  ``idx``: shorthand for ``expr[:, idx]``.  Returns
    (loglik fp64 scalar, sse_per_gene fp64 (D,), ss_per_gene fp64 (D,), dmean, dscale, dW, db, dnoise_sd), or the first three
    with ``grads=False`` (the same bits).  ``ss_per_gene`` is the null sum of squares sum_n (y - mean_n y)^2 of the batch.
    Nothing here waits for the device: the call can be captured in a graph."""
    from .likelihoods import SparseExpression
    if not isinstance(expr, SparseExpression):
        raise TypeError(f"gaussian_fa_sparse: expr must be a SparseExpression, got {type(expr).__name__}")
    if idx is not None:
        expr = expr[:, idx]
    return _gaussian_fa_sparse(mean, scale, W, b, noise_sd, expr, grads)


@_on_device
def _gaussian_fa_sparse(mean, scale, W, b, noise_sd, expr, grads):
    _need_cuda(mean, scale, W, b, noise_sd)
    dev = mean.device
    if expr.device != dev:
        raise RuntimeError(f"gpzoo_amd: the expression lives on {expr.device}, the model on {dev}: move it with expr.to(device)")
    lib = _lib.load()
    f32 = torch.float32
    mean, scale, W, b, noise_sd = (t.detach().to(f32).contiguous() for t in (mean, scale, W, b, noise_sd))
    if mean.dim() != 2:
        raise ValueError(f"gaussian_fa_sparse: mean {tuple(mean.shape)} must be (Lt, B)")
    view, base = expr.values, expr.values.base
    D, N = base.shape
    Lt, B = mean.shape
    if tuple(expr.shape) != (D, B) or scale.shape != (Lt, B) or W.shape != (D, Lt) or b.shape != (D,) or noise_sd.shape != (D,):
        raise ValueError(f"gaussian_fa_sparse: expr {tuple(expr.shape)}, mean {tuple(mean.shape)}, scale {tuple(scale.shape)}, W "
                         f"{tuple(W.shape)}, b {tuple(b.shape)}, noise_sd {tuple(noise_sd.shape)} do not fit together")
    nnz = int(base.col_val.numel())
    nb = C.c_int64()
    if lib.gpz_gaussian_fa_sparse_plan(N, B, D, Lt, nnz, None, None, None, C.byref(nb)) != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    ll = torch.empty(1, dtype=torch.float64, device=dev)
    sse = torch.empty(D, dtype=torch.float64, device=dev)
    ss = torch.empty(D, dtype=torch.float64, device=dev)
    out = [torch.empty((Lt, B), dtype=f32, device=dev), torch.empty((Lt, B), dtype=f32, device=dev),
           torch.empty((D, Lt), dtype=f32, device=dev), torch.empty((D,), dtype=f32, device=dev),
           torch.empty((D,), dtype=f32, device=dev)] if grads else [None] * 5
    ws = _workspace(dev, nb.value)
    rc = lib.gpz_gaussian_fa_sparse(_ptr(mean), _ptr(scale), _ptr(W), _ptr(b), _ptr(noise_sd), _ptr(expr.offset),
                                    _ptr(base.col_ptr), _ptr(base.col_gene), _ptr(base.col_val), _ptr(base.row_ptr),
                                    _ptr(base.row_spot), _ptr(base.row_perm), _ptr(view.idx), _ptr(view.pos), N, B, D, nnz, Lt,
                                    _ptr(ll), _ptr(sse), _ptr(ss), *(_ptr(t) for t in out), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, "gpz_gaussian_fa_sparse")
    return (ll[0], sse, ss, *out) if grads else (ll[0], sse, ss)


def gene_rank_plan(N: int, D: int, nnz: int, K: Optional[int] = None) -> dict:
    """How ``gene_deviance_sparse`` (``K=None``) or ``gene_morans_i_sparse`` (``K`` neighbours) covers a shape
    (gpz_gene_deviance_sparse_plan / gpz_gene_morans_i_sparse_plan, host-only queries: no device needed): ``gene_chunk``
    (stored entries of a gene row per sweep of its workgroup), ``workgroups`` (genes in flight), ``partials_bytes``."""
    lib = _lib.load()
    gc, wg, nb = C.c_int32(), C.c_int32(), C.c_int64()
    if K is None:
        rc = lib.gpz_gene_deviance_sparse_plan(int(N), int(D), int(nnz), C.byref(gc), C.byref(wg), C.byref(nb))
    else:
        rc = lib.gpz_gene_morans_i_sparse_plan(int(N), int(D), int(nnz), int(K), C.byref(gc), C.byref(wg), C.byref(nb))
    if rc != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return dict(gene_chunk=gc.value, workgroups=wg.value, partials_bytes=int(nb.value))


def _whole_values(values, who: str):
    """The whole ``SparseCounts``-structured object behind ``values`` (itself, or the values of a ``SparseExpression``)."""
    from .likelihoods import SparseCounts, SparseExpression
    if isinstance(values, SparseExpression):
        values = values.values
    if not isinstance(values, SparseCounts):
        raise TypeError(f"{who}: a SparseCounts or a SparseExpression expected, got {type(values).__name__}")
    if values.base is not values:
        raise TypeError(f"{who}: a view y[:, idx]; the whole data set is needed")
    return values


def gene_deviance_sparse(counts, size, family: int = 0):
    """Per-gene (sum, count, deviance), fp64 (D,) each, of a whole ``SparseCounts`` against the constant-rate null
    (gpz_gene_deviance_sparse): ``size`` (N,) fp64 on the counts' device, positive wherever a spot has a stored count;
    ``family`` 0 Poisson, 1 binomial (``size`` = the spots' totals).  Nothing here waits for the device."""
    from .likelihoods import SparseCounts, _counts_expected
    _counts_expected(counts, "gene_deviance_sparse")
    if not isinstance(counts, SparseCounts):
        raise TypeError(f"gene_deviance_sparse: counts must be a SparseCounts, got {type(counts).__name__}")
    c = _whole_values(counts, "gene_deviance_sparse")
    _need_cuda(c.col_val)
    if family not in (0, 1):
        raise ValueError(f"gene_deviance_sparse: family {family!r} unknown (0 Poisson, 1 binomial)")
    D, N = c.shape
    if not isinstance(size, torch.Tensor) or size.dtype != torch.float64 or tuple(size.shape) != (N,):
        raise ValueError(f"gene_deviance_sparse: size must be an ({N},) float64 tensor")
    if size.device != c.device:
        raise RuntimeError(f"gpzoo_amd: the counts live on {c.device}, size on {size.device}")
    return _gene_deviance_sparse(c, size.detach().contiguous(), int(family))


def _gene_deviance_sparse(c, size, family):
    lib = _lib.load()
    dev = c.device
    D, N = c.shape
    nb = C.c_int64()
    if lib.gpz_gene_deviance_sparse_plan(N, D, c.nnz, None, None, C.byref(nb)) != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    out = [torch.empty(D, dtype=torch.float64, device=dev) for _ in range(3)]
    with torch.cuda.device(dev):
        ws = _workspace(dev, nb.value)
        rc = lib.gpz_gene_deviance_sparse(_ptr(c.row_ptr), _ptr(c.row_spot), _ptr(c.row_perm), _ptr(c.col_val), _ptr(size), N, D,
                                          c.nnz, family, *(_ptr(t) for t in out), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, "gpz_gene_deviance_sparse")
    return tuple(out)


def _nbr_table(who: str, nbr, N: int, dev):
    """The (N, K) neighbour table of a gene entry as contiguous int64 on ``dev``, and K."""
    if not isinstance(nbr, torch.Tensor) or nbr.dim() != 2 or nbr.shape[0] != N or nbr.dtype.is_floating_point:
        raise ValueError(f"{who}: nbr must be an ({N}, K) integer table")
    return nbr.to(device=dev, dtype=torch.int64).contiguous(), int(nbr.shape[1])


def gene_morans_i_sparse(values, nbr) -> torch.Tensor:
    """(D,) fp64 Moran's I of every gene of a whole ``SparseCounts`` / ``SparseExpression`` (the offset does not change I)
    over the neighbour table nbr (N,K) int64, 1 <= K <= 32, with row-normalised weights (gpz_gene_morans_i_sparse): what
    ``morans_i`` gives for the dense transpose, zeros included, from sums over the stored entries.  NaN for a gene without
    stored entries and for a constant one.  A table entry outside [0, N) or naming its own row raises ValueError (checked
    on the device; one synchronisation)."""
    v = _whole_values(values, "gene_morans_i_sparse")
    _need_cuda(v.col_val)
    D, N = v.shape
    dev = v.device
    nbr, K = _nbr_table("gene_morans_i_sparse", nbr, N, dev)
    lib = _lib.load()
    nb = C.c_int64()
    if lib.gpz_gene_morans_i_sparse_plan(N, D, v.nnz, K, None, None, C.byref(nb)) != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    out = torch.empty(D, dtype=torch.float64, device=dev)
    info = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws = _workspace(dev, nb.value)
        rc = lib.gpz_gene_morans_i_sparse(_ptr(v.row_ptr), _ptr(v.row_spot), _ptr(v.row_perm), _ptr(v.col_val), _ptr(nbr), N, D,
                                          v.nnz, K, _ptr(out), _ptr(info), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, "gpz_gene_morans_i_sparse")
    if int(info.item()) != 0:
        raise ValueError("gene_morans_i_sparse: the neighbour table has an entry outside [0, N) or naming its own row")
    return out


_LINE_MODES = {0: 0, 1: 1, 2: 2, "auto": 0, "global": 1, "lds": 2}


def _line_mode(who: str, line_mode) -> int:
    if isinstance(line_mode, bool) or line_mode not in _LINE_MODES:
        raise ValueError(f"{who}: line_mode {line_mode!r} unknown (0 / 'auto', 1 / 'global', 2 / 'lds')")
    return _LINE_MODES[line_mode]


def _perm_plan(who: str, family: str, stat, N, D, K, P, nnz, perm_batch, line_mode) -> dict:
    """The plan query of a permutation entry: ``family`` "morans" (``stat`` None) or "autocorr" (``stat`` 0 or 1), rows stored
    as their non-zeros (``nnz``) or dense (``nnz=None``)."""
    lib = _lib.load()
    pb, lm, wg, nb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    entry = f"gpz_{family}_perm_rows_plan" if nnz is None else f"gpz_gene_{family}_perm_sparse_plan"
    extents = [int(N), int(D)] if nnz is None else [int(N), int(D), int(nnz)]
    batch = [int(K), int(P)] if stat is None else [int(K), int(P), stat]
    rc = getattr(lib, entry)(*extents, *batch, int(perm_batch), _line_mode(who, line_mode), C.byref(pb), C.byref(lm), C.byref(wg),
                             C.byref(nb))
    if rc != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return dict(perm_batch=pb.value, line_mode=lm.value, workgroups=wg.value, partials_bytes=int(nb.value))


def morans_perm_plan(N: int, D: int, K: int, P: int, nnz: Optional[int] = None, perm_batch: int = 0, line_mode=0) -> dict:
    """How ``gene_morans_perm_sparse`` (``nnz`` stored entries) or ``morans_perm_rows`` (``nnz=None``) covers a shape
    (gpz_gene_morans_perm_sparse_plan / gpz_morans_perm_rows_plan, host-only queries: no device needed): ``perm_batch``
    (permutations per launch) and ``line_mode`` (1 scratch memory, 2 LDS) as resolved, ``workgroups`` (genes in flight),
    ``partials_bytes``.  A ``line_mode`` of 2 where a line of N floats does not fit the LDS raises ValueError."""
    return _perm_plan("morans_perm_plan", "morans", None, N, D, K, P, nnz, perm_batch, line_mode)


def _perm_table_check(who: str, perms, N: int, perm_batch) -> None:
    """What the permutation entries check of ``perms`` and ``perm_batch`` before any device work."""
    if (not isinstance(perms, torch.Tensor) or perms.dim() != 2 or perms.shape[0] < 1 or perms.shape[1] != N
            or perms.dtype.is_floating_point or perms.dtype == torch.bool):
        raise ValueError(f"{who}: perms must be a (P, {N}) integer tensor, P >= 1")
    if isinstance(perm_batch, bool) or not isinstance(perm_batch, int) or perm_batch < 0:
        raise ValueError(f"{who}: perm_batch {perm_batch!r} must be a non-negative integer (0 = chosen by the plan)")


def _perm_table(perms, N: int, dev):
    """``perms`` as contiguous int32 on ``dev``."""
    if perms.dtype != torch.int32:
        perms = perms.to(device=dev, dtype=torch.int64).clamp(-1, N)                  # a wide entry stays out of range in 32 bits
    return perms.to(device=dev, dtype=torch.int32).contiguous()


def _morans_perm(who: str, family: str, stat, N: int, D: int, nnz, dev, inputs, nbr, perms, return_sims, perm_batch, line_mode):
    """The call behind the four permutation entries, named as ``_perm_plan`` names them: ``family`` "autocorr" with ``stat``
    0 (Moran) or 1 (Geary), "morans" with None; ``inputs`` are the entry's leading pointers.  Returns the tensors of a
    ``MoransPerm`` in its order."""
    nbr, K = _nbr_table(who, nbr, N, dev)
    _perm_table_check(who, perms, N, perm_batch)
    perms = _perm_table(perms, N, dev)
    P = int(perms.shape[0])
    plan = _perm_plan(who, family, stat, N, D, K, P, nnz, perm_batch, line_mode)
    entry = f"gpz_{family}_perm_rows" if nnz is None else f"gpz_gene_{family}_perm_sparse"
    extents = [N, D] if nnz is None else [N, D, nnz]
    batch = [K, P] if stat is None else [K, P, stat]
    lib = _lib.load()
    I, mean, m2 = (torch.empty(D, dtype=torch.float64, device=dev) for _ in range(3))
    n_ge, n_le = (torch.empty(D, dtype=torch.int32, device=dev) for _ in range(2))
    sims = torch.empty((D, P), dtype=torch.float64, device=dev) if return_sims else None
    info = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws = _workspace(dev, plan["partials_bytes"])
        rc = getattr(lib, entry)(*inputs, _ptr(nbr), _ptr(perms), *extents, *batch, plan["perm_batch"], plan["line_mode"], _ptr(I),
                                 _ptr(sims), _ptr(n_ge), _ptr(n_le), _ptr(mean), _ptr(m2), _ptr(info), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, entry)
    code = int(info.item())
    if code == 1:
        raise ValueError(f"{who}: the neighbour table has an entry outside [0, N) or naming its own row")
    if code != 0:
        raise ValueError(f"{who}: a row of perms is not a permutation of 0 .. N - 1 (an entry outside [0, N) or an index named twice)")
    return I, n_ge, n_le, mean, m2, sims


@dataclass
class MoransPerm:
    """``gene_morans_perm_sparse`` / ``morans_perm_rows``: ``I`` (D,) fp64; ``n_ge`` / ``n_le`` (D,) int32, the permutations
    with I_pi >= I / <= I; ``sim_mean`` and ``sim_m2`` (D,) fp64, the mean of I_pi and sum (I_pi - mean)^2; ``sims`` (D, P)
    fp64 or None."""
    I: torch.Tensor
    n_ge: torch.Tensor
    n_le: torch.Tensor
    sim_mean: torch.Tensor
    sim_m2: torch.Tensor
    sims: Optional[torch.Tensor]


def gene_morans_perm_sparse(values, nbr, perms, *, return_sims: bool = False, perm_batch: int = 0, line_mode=0) -> MoransPerm:
    """Moran's I of every gene of a whole ``SparseCounts`` / ``SparseExpression`` under the P relabellings of the spots in
    ``perms`` (P, N) integer, x^pi[i] = x[pi[i]], over nbr (N,K) int64, 1 <= K <= 32 (gpz_gene_morans_perm_sparse): ``I`` is
    ``gene_morans_i_sparse``'s, bit for bit; the counts compare N C - S A in fp64, exact for integer-valued data.  A
    ``MoransPerm``; all of it is independent of ``perm_batch`` (permutations per launch, 0 = the plan's) and ``line_mode``
    (0 / "auto", 1 / "global", 2 / "lds").  A bad neighbour table and a row of ``perms`` that is no permutation raise
    ValueError (checked on the device; one synchronisation)."""
    who = "gene_morans_perm_sparse"
    v = _whole_values(values, who)
    _need_cuda(v.col_val)
    D, N = v.shape
    inputs = (_ptr(v.row_ptr), _ptr(v.row_spot), _ptr(v.row_perm), _ptr(v.col_val))
    return MoransPerm(*_morans_perm(who, "morans", None, N, D, v.nnz, v.device, inputs, nbr, perms, return_sims, perm_batch, line_mode))


def morans_perm_rows(values, nbr, perms, *, return_sims: bool = False, perm_batch: int = 0, line_mode=0) -> MoransPerm:
    """``gene_morans_perm_sparse`` for a dense fp32 (D, N) tensor, one gene per row (gpz_morans_perm_rows): every spot is an
    entry, zeros included, and the row is its own line.  ``I`` is the expanded form's, within rounding of ``morans_i`` of the
    transpose."""
    who = "morans_perm_rows"
    if not isinstance(values, torch.Tensor) or values.dim() != 2 or values.dtype != torch.float32:
        raise ValueError(f"{who}: a dense (D, N) float32 tensor expected")
    _need_cuda(values)
    V = values.detach().contiguous()
    D, N = V.shape
    return MoransPerm(*_morans_perm(who, "morans", None, N, D, None, V.device, (_ptr(V),), nbr, perms, return_sims, perm_batch, line_mode))


_STATS = {"moran": 0, "geary": 1}


def _stat(who: str, stat) -> int:
    if not isinstance(stat, str) or stat not in ("moran", "geary"):
        raise ValueError(f"{who}: stat {stat!r} unknown ('moran', 'geary')")
    return _STATS[stat]


@dataclass
class SpatialStats:
    """``gene_spatial_stats_sparse`` / ``spatial_stats``, fp64 per gene / column: Moran's ``I``, Geary's ``C``, ``mean``,
    ``var`` (the population variance m2, zeros included) and ``kurtosis`` (b2 = m4 / m2^2)."""
    I: torch.Tensor
    C: torch.Tensor
    mean: torch.Tensor
    var: torch.Tensor
    kurtosis: torch.Tensor


def spatial_stats_plan(N: int, K: int, D: Optional[int] = None, nnz: Optional[int] = None, L: Optional[int] = None) -> dict:
    """How ``gene_spatial_stats_sparse`` (``D`` genes, ``nnz`` stored entries) or ``spatial_stats`` (``L`` columns) covers a
    shape (gpz_gene_spatial_stats_sparse_plan / gpz_spatial_stats_plan, host-only queries: no device needed):
    ``gene_chunk``, ``workgroups``, ``partials_bytes``, or ``row_chunk``, ``chunks``, ``partials_bytes``."""
    lib = _lib.load()
    nb = C.c_int64()
    if L is not None:
        rc_, ch = C.c_int32(), C.c_int64()
        if lib.gpz_spatial_stats_plan(int(N), int(L), int(K), C.byref(rc_), C.byref(ch), C.byref(nb)) != 0:
            raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
        return dict(row_chunk=rc_.value, chunks=int(ch.value), partials_bytes=int(nb.value))
    gc, wg = C.c_int32(), C.c_int32()
    if lib.gpz_gene_spatial_stats_sparse_plan(int(N), int(D), int(nnz), int(K), C.byref(gc), C.byref(wg), C.byref(nb)) != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return dict(gene_chunk=gc.value, workgroups=wg.value, partials_bytes=int(nb.value))


def gene_spatial_stats_sparse(values, nbr) -> SpatialStats:
    """Moran's I, Geary's C, the mean, the variance and the kurtosis of every gene of a whole ``SparseCounts`` /
    ``SparseExpression`` over the neighbour table nbr (N,K) int64 of distinct neighbours, 1 <= K <= 32
    (gpz_gene_spatial_stats_sparse), from sums over the stored entries, zeros included: a ``SpatialStats`` of (D,) fp64
    tensors.  ``I`` is ``gene_morans_i_sparse``'s, bit for bit.  The offset of a ``SparseExpression`` moves the mean and
    nothing else.  I, C and the kurtosis are NaN for a gene without stored entries and for a constant one.  A table entry
    outside [0, N) or naming its own row raises ValueError (checked on the device; one synchronisation)."""
    from .likelihoods import SparseExpression
    who = "gene_spatial_stats_sparse"
    v = _whole_values(values, who)
    _need_cuda(v.col_val)
    D, N = v.shape
    dev = v.device
    nbr, K = _nbr_table(who, nbr, N, dev)
    plan = spatial_stats_plan(N, K, D=D, nnz=v.nnz)
    lib = _lib.load()
    out = [torch.empty(D, dtype=torch.float64, device=dev) for _ in range(5)]
    info = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws = _workspace(dev, plan["partials_bytes"])
        rc = lib.gpz_gene_spatial_stats_sparse(_ptr(v.row_ptr), _ptr(v.row_spot), _ptr(v.row_perm), _ptr(v.col_val), _ptr(nbr), N, D,
                                               v.nnz, K, *(_ptr(t) for t in out), _ptr(info), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, "gpz_gene_spatial_stats_sparse")
    if int(info.item()) != 0:
        raise ValueError(f"{who}: the neighbour table has an entry outside [0, N) or naming its own row")
    if isinstance(values, SparseExpression):
        out[2] = out[2] - values.offset.to(device=dev, dtype=torch.float64)
    return SpatialStats(*out)


@_on_device
def spatial_stats(values, nbr) -> SpatialStats:
    """``gene_spatial_stats_sparse`` for the columns of values (N,L), fp32 or fp64, as ``morans_i`` takes them
    (gpz_spatial_stats): a ``SpatialStats`` of (L,) fp64 tensors from centred sums; ``I`` is ``morans_i``'s, bit for bit.  A
    constant column gives NaN in I, C and the kurtosis."""
    _need_cuda(values)
    V = values.detach().contiguous()
    if V.dim() != 2 or nbr.dim() != 2 or nbr.shape[0] != V.shape[0]:
        raise ValueError(f"spatial_stats: values (N, L) and nbr (N, K) expected, got {tuple(V.shape)} and {tuple(nbr.shape)}")
    nbr = nbr.to(device=V.device, dtype=torch.int64).contiguous()
    N, L = V.shape
    K = nbr.shape[1]
    plan = spatial_stats_plan(N, K, L=L)
    lib = _lib.load()
    out = [torch.empty(L, dtype=torch.float64, device=V.device) for _ in range(5)]
    info = torch.empty(1, dtype=torch.int32, device=V.device)
    ws = _workspace(V.device, plan["partials_bytes"])
    rc = lib.gpz_spatial_stats(_ptr(V), N, L, _dt(V), _ptr(nbr), K, *(_ptr(t) for t in out), _ptr(info), _ptr(ws), ws.numel(),
                               _stream(V.device))
    _lib.check(rc, "gpz_spatial_stats")
    if int(info.item()) != 0:
        raise ValueError("spatial_stats: the neighbour table has an entry outside [0, N) or naming its own row")
    return SpatialStats(*out)


def autocorr_perm_plan(N: int, D: int, K: int, P: int, nnz: Optional[int] = None, stat: str = "moran", perm_batch: int = 0,
                       line_mode=0) -> dict:
    """``morans_perm_plan`` for ``gene_autocorr_perm_sparse`` (``nnz`` stored entries) or ``autocorr_perm_rows``
    (``nnz=None``) (gpz_gene_autocorr_perm_sparse_plan / gpz_autocorr_perm_rows_plan, host-only queries)."""
    return _perm_plan("autocorr_perm_plan", "autocorr", _stat("autocorr_perm_plan", stat), N, D, K, P, nnz, perm_batch, line_mode)


@dataclass
class AutocorrPerm:
    """``gene_autocorr_perm_sparse`` / ``autocorr_perm_rows``: ``stat`` ("moran" or "geary"); ``value`` (D,) fp64, the
    observed I or C; ``n_ge`` / ``n_le`` (D,) int32, the permutations whose statistic is >= / <= the observed one;
    ``sim_mean`` and ``sim_m2`` (D,) fp64, the mean of the simulated statistic and the sum of its squared deviations;
    ``sims`` (D, P) fp64 or None."""
    stat: str
    value: torch.Tensor
    n_ge: torch.Tensor
    n_le: torch.Tensor
    sim_mean: torch.Tensor
    sim_m2: torch.Tensor
    sims: Optional[torch.Tensor]


def gene_autocorr_perm_sparse(values, nbr, perms, *, stat: str = "moran", return_sims: bool = False, perm_batch: int = 0,
                              line_mode=0) -> AutocorrPerm:
    """``gene_morans_perm_sparse`` with the statistic as an argument (gpz_gene_autocorr_perm_sparse): ``stat="moran"`` gives
    its bits; ``stat="geary"`` Geary's C of every gene (``gene_spatial_stats_sparse``'s, bit for bit) and of its P
    relabellings, compared on Q_in - 2 C_s in fp64, exact for integer-valued data.  An ``AutocorrPerm``."""
    who = "gene_autocorr_perm_sparse"
    st = _stat(who, stat)
    v = _whole_values(values, who)
    _need_cuda(v.col_val)
    D, N = v.shape
    inputs = (_ptr(v.row_ptr), _ptr(v.row_spot), _ptr(v.row_perm), _ptr(v.col_val))
    return AutocorrPerm(stat, *_morans_perm(who, "autocorr", st, N, D, v.nnz, v.device, inputs, nbr, perms, return_sims, perm_batch,
                                            line_mode))


def autocorr_perm_rows(values, nbr, perms, *, stat: str = "moran", return_sims: bool = False, perm_batch: int = 0,
                       line_mode=0) -> AutocorrPerm:
    """``gene_autocorr_perm_sparse`` for a dense fp32 (D, N) tensor, one gene per row (gpz_autocorr_perm_rows): every spot is
    an entry, zeros included; ``stat="moran"`` gives the bits of ``morans_perm_rows``."""
    who = "autocorr_perm_rows"
    st = _stat(who, stat)
    if not isinstance(values, torch.Tensor) or values.dim() != 2 or values.dtype != torch.float32:
        raise ValueError(f"{who}: a dense (D, N) float32 tensor expected")
    _need_cuda(values)
    V = values.detach().contiguous()
    D, N = V.shape
    return AutocorrPerm(stat, *_morans_perm(who, "autocorr", st, N, D, None, V.device, (_ptr(V),), nbr, perms, return_sims, perm_batch,
                                            line_mode))


def gene_dispersion_plan(N: int, D: int, nnz: int) -> dict:
    """How ``gene_dispersion_sparse`` covers a shape (gpz_gene_dispersion_sparse_plan, a host-only query: no device needed):
    ``gene_chunk`` (stored entries of a gene row per sweep of its workgroup), ``workgroups`` (genes in flight), ``tol_t`` (the
    solver stops at a step or bracket of this size in log theta), ``partials_bytes``."""
    lib = _lib.load()
    gc, wg, tol, nb = C.c_int32(), C.c_int32(), C.c_double(), C.c_int64()
    if lib.gpz_gene_dispersion_sparse_plan(int(N), int(D), int(nnz), C.byref(gc), C.byref(wg), C.byref(tol), C.byref(nb)) != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return dict(gene_chunk=gc.value, workgroups=wg.value, tol_t=tol.value, partials_bytes=int(nb.value))


def gene_dispersion_sparse(counts, size, theta_min: float = 1e-4, theta_max: float = 1e6, max_iter: int = 50):
    """Per-gene (theta, gain, poisson_loglik, status, iterations) of a whole ``SparseCounts``: the maximum-likelihood
    negative-binomial inverse dispersion under the constant-rate null mu_n = p size_n, p = sum y / sum size
    (gpz_gene_dispersion_sparse; include/gpzoo_hip.h has the statistic).  ``size`` (N,) fp64 on the counts' device, >= 0 and
    positive wherever a spot has a stored count.  theta, gain, poisson_loglik fp64 (D,), status and iterations int32 (D,):
    status 0 an interior root, 1 theta = +inf (no overdispersion below ``theta_max``; gain 0), 2 ``theta_min``, 3 not
    converged in ``max_iter`` <= 200 score evaluations (``max_iter=0``: the moment start), 4 a gene without counts (NaN).
    A stored value that is negative or not an integer, or a bad size, raises ValueError (checked on the device; one
    synchronisation)."""
    import math
    from .likelihoods import SparseCounts, _counts_expected
    who = "gene_dispersion_sparse"
    _counts_expected(counts, who)
    if not isinstance(counts, SparseCounts):
        raise TypeError(f"{who}: counts must be a SparseCounts, got {type(counts).__name__}")
    c = _whole_values(counts, who)
    theta_min, theta_max = float(theta_min), float(theta_max)
    if not (0.0 < theta_min < theta_max and math.isfinite(theta_max)):
        raise ValueError(f"{who}: theta range ({theta_min}, {theta_max}) unsupported (0 < theta_min < theta_max, both finite)")
    if int(max_iter) != max_iter or not 0 <= int(max_iter) <= 200:
        raise ValueError(f"{who}: max_iter = {max_iter!r} outside [0, 200]")
    D, N = c.shape
    if not isinstance(size, torch.Tensor) or size.dtype != torch.float64 or tuple(size.shape) != (N,):
        raise ValueError(f"{who}: size must be an ({N},) float64 tensor")
    _need_cuda(c.col_val)
    if size.device != c.device:
        raise RuntimeError(f"gpzoo_amd: the counts live on {c.device}, size on {size.device}")
    size = size.detach().contiguous()
    lib = _lib.load()
    dev = c.device
    nb = C.c_int64()
    if lib.gpz_gene_dispersion_sparse_plan(N, D, c.nnz, None, None, None, C.byref(nb)) != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    out = [torch.empty(D, dtype=torch.float64, device=dev) for _ in range(3)]
    out += [torch.empty(D, dtype=torch.int32, device=dev) for _ in range(2)]
    info = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws = _workspace(dev, nb.value)
        rc = lib.gpz_gene_dispersion_sparse(_ptr(c.row_ptr), _ptr(c.row_spot), _ptr(c.row_perm), _ptr(c.col_val), _ptr(size), N, D,
                                            c.nnz, theta_min, theta_max, int(max_iter), *(_ptr(t) for t in out), _ptr(info),
                                            _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, "gpz_gene_dispersion_sparse")
    flags = int(info.item())
    if flags & 1:
        raise ValueError(f"{who}: a stored value is negative, not an integer or >= 2^24 (counts expected)")
    if flags & 2:
        raise ValueError(f"{who}: size must be >= 0 and finite, and positive wherever a spot has a stored count")
    return tuple(out)


GENE_GP_KINDS = {"rbf": _lib.KERNEL_RBF, "matern12": _lib.KERNEL_MATERN12, "matern32": _lib.KERNEL_MATERN32,
                 "matern52": _lib.KERNEL_MATERN52}


def gene_kernel_project_plan(N: int, D: int, nnz: int, M: int, n_ell: int) -> dict:
    """How ``gene_kernel_project_sparse`` covers a shape (gpz_gene_kernel_project_sparse_plan, a host-only query: no device
    needed): ``gene_chunk`` (a gene row longer than this many stored entries is cut into chunks of that many, whose sums
    are folded in order), ``workgroups`` (along the genes), ``generate`` (True while generating the covariances in the
    kernel is the faster way; above 290 N stored entries ``gene_kernel_project_gather`` is), ``partials_bytes``."""
    lib = _lib.load()
    gc, wg, gen, nb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    if lib.gpz_gene_kernel_project_sparse_plan(int(N), int(D), int(nnz), int(M), int(n_ell), C.byref(gc), C.byref(wg),
                                               C.byref(gen), C.byref(nb)) != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return dict(gene_chunk=gc.value, workgroups=wg.value, generate=bool(gen.value), partials_bytes=int(nb.value))


def _gene_gp_kind(who, kernel):
    if kernel not in GENE_GP_KINDS:
        raise ValueError(f"{who}: kernel {kernel!r} unknown ({', '.join(repr(k) for k in GENE_GP_KINDS)})")
    return GENE_GP_KINDS[kernel]


def gene_kernel_project_sparse(values, coords, Z, lengthscales, kernel: str = "rbf", *, workgroups: int = 0, partials=None):
    """``out[l, g, m] = sum_{stored (g, n)} v_gn k_l(z_m, x_n)``, fp64 (n_ell, D, M): K_zx Y^T of every gene of a whole
    ``SparseCounts`` / ``SparseExpression`` (its stored values; the offset is the caller's) for the unit-variance ``kernel``
    ("rbf", "matern12", "matern32", "matern52") at every length scale (gpz_gene_kernel_project_sparse).  ``coords`` (N, d),
    ``Z`` (M, d), ``lengthscales`` (n_ell,) fp64 tensors on the values' device; d <= 4, M <= 1024, n_ell <= 16.  The
    covariances are generated in the kernel and never stored.  ``workgroups`` (0: the plan's) does not change a bit of the
    result.  ``partials``: a uint8 scratch tensor of the plan's ``partials_bytes`` to use in place of the shared one."""
    who = "gene_kernel_project_sparse"
    kind = _gene_gp_kind(who, kernel)
    v = _whole_values(values, who)
    D, N = v.shape
    for name, t in (("coords", coords), ("Z", Z), ("lengthscales", lengthscales)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
            raise ValueError(f"{who}: {name} must be a float64 tensor")
    if coords.dim() != 2 or Z.dim() != 2 or lengthscales.dim() != 1 or coords.shape[0] != N or Z.shape[1] != coords.shape[1]:
        raise ValueError(f"{who}: coords ({N}, d), Z (M, d) and lengthscales (n_ell,) expected, got {tuple(coords.shape)}, "
                         f"{tuple(Z.shape)} and {tuple(lengthscales.shape)}")
    _need_cuda(v.col_val)
    dev = v.device
    for name, t in (("coords", coords), ("Z", Z), ("lengthscales", lengthscales)):
        if t.device != dev:
            raise RuntimeError(f"gpzoo_amd: the values live on {dev}, {name} on {t.device}")
    X, Zc, ell = coords.detach().contiguous(), Z.detach().contiguous(), lengthscales.detach().contiguous()
    M, d, nl = int(Zc.shape[0]), int(Zc.shape[1]), int(ell.numel())
    lib = _lib.load()
    nb = C.c_int64()
    if lib.gpz_gene_kernel_project_sparse_plan(N, D, v.nnz, M, nl, None, None, None, C.byref(nb)) != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    out = torch.empty((nl, D, M), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        ws = _workspace(dev, nb.value) if partials is None else partials
        rc = lib.gpz_gene_kernel_project_sparse(_ptr(v.row_ptr), _ptr(v.row_spot), _ptr(v.row_perm), _ptr(v.col_val), _ptr(X),
                                                _ptr(Zc), _ptr(ell), N, D, v.nnz, M, d, nl, kind, int(workgroups), _ptr(out),
                                                _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, "gpz_gene_kernel_project_sparse")
    return out


def gene_kernel_project_gather(values, coords, Z, lengthscales, kernel: str = "rbf"):
    """What ``gene_kernel_project_sparse`` computes, composed from a stored K_xz: per length scale ``kfill`` of the fp64
    (N, M) covariance and ``counts_matmul`` of the stored values with it in column blocks of 128.  It allocates N x M x 8
    bytes at a time and adds in ``counts_matmul``'s order; above the density where the plan's ``generate`` turns False it
    is the faster of the two (one multiply-add per gathered covariance instead of an exp)."""
    who = "gene_kernel_project_gather"
    kind = _gene_gp_kind(who, kernel)
    v = _whole_values(values, who)
    _need_cuda(v.col_val)
    D = v.shape[0]
    X, Zc, ell = coords.detach().contiguous(), Z.detach().contiguous(), lengthscales.detach().contiguous()
    M, nl = int(Zc.shape[0]), int(ell.numel())
    out = torch.empty((nl, D, M), dtype=torch.float64, device=v.device)
    one = torch.ones(1, dtype=torch.float64, device=v.device)
    for l in range(nl):
        Kxz = kfill(KernelSpec(kind, one, ell[l:l + 1], False), X, Zc)
        for m0 in range(0, M, 128):
            out[l, :, m0:m0 + 128] = counts_matmul(v, Kxz[:, m0:m0 + 128].contiguous(), transpose=True)
    return out


def gene_gp_profile_plan(D: int, M: int, n_ell: int) -> dict:
    """How ``gene_gp_profile`` maximises (gpz_gene_gp_profile_plan, a host-only query): ``grid_points`` (values of log
    delta the bound is evaluated at first), ``workgroups``, ``tol_t`` (the refinement stops at a step or bracket of this
    size in log delta), ``max_iter``."""
    lib = _lib.load()
    gp, wg, tol, mi = C.c_int32(), C.c_int32(), C.c_double(), C.c_int32()
    if lib.gpz_gene_gp_profile_plan(int(D), int(M), int(n_ell), C.byref(gp), C.byref(wg), C.byref(tol), C.byref(mi)) != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return dict(grid_points=gp.value, workgroups=wg.value, tol_t=tol.value, max_iter=mi.value)


def gene_gp_profile(p, lam, yty, N: int, delta_min: float = 1e-3, delta_max: float = 1e6):
    """Per (gene, length scale) the maximum over delta = tau / s of the collapsed sparse-GP bound with s profiled out
    (gpz_gene_gp_profile; include/gpzoo_hip.h has the statistic): ``p`` (n_ell, D, M) the rotated projections U^T Phi y,
    ``lam`` (n_ell, M) the eigenvalues of Phi Phi^T, ``yty`` (D,), fp64 on one device; N spots.  Returns ``(loglik, delta,
    s2, tau2, status, iterations)``, (D, n_ell) each, fp64 and int32: status 0 interior, 1 no spatial variance in range
    (the values at ``delta_max``), 2 at ``delta_min``, 3 degenerate (NaN)."""
    import math
    who = "gene_gp_profile"
    for name, t in (("p", p), ("lam", lam), ("yty", yty)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
            raise ValueError(f"{who}: {name} must be a float64 tensor")
    if p.dim() != 3 or tuple(lam.shape) != (p.shape[0], p.shape[2]) or tuple(yty.shape) != (p.shape[1],):
        raise ValueError(f"{who}: p (n_ell, D, M), lam (n_ell, M) and yty (D,) expected, got {tuple(p.shape)}, {tuple(lam.shape)} "
                         f"and {tuple(yty.shape)}")
    delta_min, delta_max = float(delta_min), float(delta_max)
    if not (0.0 < delta_min < delta_max and math.isfinite(delta_max)):
        raise ValueError(f"{who}: delta range ({delta_min}, {delta_max}) unsupported (0 < delta_min < delta_max, both finite)")
    _need_cuda(p, lam, yty)
    dev = _same_device(p, lam, yty)
    nl, D, M = (int(s) for s in p.shape)
    p, lam, yty = p.detach().contiguous(), lam.detach().contiguous(), yty.detach().contiguous()
    lib = _lib.load()
    out = [torch.empty((D, nl), dtype=torch.float64, device=dev) for _ in range(4)]
    out += [torch.empty((D, nl), dtype=torch.int32, device=dev) for _ in range(2)]
    with torch.cuda.device(dev):
        rc = lib.gpz_gene_gp_profile(_ptr(p), _ptr(lam), _ptr(yty), int(N), D, M, nl, delta_min, delta_max,
                                     *(_ptr(t) for t in out), _stream(dev))
    _lib.check(rc, "gpz_gene_gp_profile")
    return tuple(out)


RESIDUAL_KINDS = {"pearson": 0, "deviance": 1}
GAUSSIAN_RESIDUAL_KINDS = {"pearson": 0, "response": 1, "predictive": 2}


def _plan_query(entry: str, args, **outs) -> dict:
    """A host-only plan query of the library: ``entry(*args, &out ...)``.  ``outs`` names the outputs in the entry's order
    and gives each its ctypes type; returns their values under those names.  A refusal raises ValueError with the entry's
    message."""
    lib = _lib.load()
    cells = {k: t() for k, t in outs.items()}
    if getattr(lib, entry)(*(int(x) for x in args), *(C.byref(c) for c in cells.values())) != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return {k: int(c.value) for k, c in cells.items()}


def residual_autocorr_plan(B: int, D: int, Lt: int, nnz: int = 0, slab_genes: int = 0) -> dict:
    """How ``residual_morans_i`` covers B spots and D scored genes (gpz_residual_morans_i_plan, a host-only query: no device
    needed): ``slab_genes`` (columns of the spot-major fp32 residual slab: the largest multiple of 64 within 256 MiB, at least
    64 and at most D rounded up to 64, or the caller's positive multiple of 64) and ``n_slabs``; the residual pass's
    ``spots_per_tile``, ``genes_per_block``, ``spot_slices`` and ``factors_padded``; ``gene_chunk`` (stored entries of a gene
    row per wave, sparse counts); ``partials_bytes`` (the scratch, slab included)."""
    i32, i64 = C.c_int32, C.c_int64
    return _plan_query("gpz_residual_morans_i_plan", (B, D, Lt, nnz, slab_genes), slab_genes=i64, n_slabs=i64, spots_per_tile=i32,
                       genes_per_block=i32, spot_slices=i32, gene_chunk=i32, factors_padded=i32, partials_bytes=i64)


def residual_autocorr_perm_plan(B: int, D: int, Lt: int, K: int, P: int, nnz: int = 0, slab_genes: int = 0,
                                perm_batch: int = 0) -> dict:
    """How ``residual_autocorr_perm`` covers B spots, D scored genes and P permutations over K neighbours
    (gpz_residual_autocorr_perm_plan, a host-only query: no device needed): ``slab_genes`` and ``n_slabs`` as
    ``residual_autocorr_plan`` gives them; ``perm_batch``, the permutations per launch as resolved (the caller's 1..32, or
    the plan's choice, whose relabelled tables of 4 B K bytes each stay within 256 MiB); ``batches`` per slab;
    ``partials_bytes``: the slab, plus O(perm_batch B K) table bytes, plus O(B / 256 x perm_batch x slab_genes) partial
    sums.  ``P=0`` asks for what ``residual_spatial_stats`` needs: no tables, ``perm_batch`` = ``batches`` = 0."""
    i32, i64 = C.c_int32, C.c_int64
    return _plan_query("gpz_residual_autocorr_perm_plan", (B, D, Lt, K, P, nnz, slab_genes, perm_batch), slab_genes=i64,
                       n_slabs=i64, perm_batch=i32, batches=i64, partials_bytes=i64)


def gaussian_residual_plan(B: int, D: int, Lt: int, K: int = 0, P: int = 0, nnz: int = 0, slab_genes: int = 0,
                           perm_batch: int = 0) -> dict:
    """How the Gaussian residual entries cover B spots, D scored genes, K neighbours and P permutations
    (gpz_gaussian_residual_plan, a host-only query: no device needed): ``slab_genes``, ``n_slabs``, ``perm_batch``,
    ``batches`` and ``partials_bytes`` as ``residual_autocorr_perm_plan`` gives them, with the residual pass's ``spot_slices``
    and ``factors_padded``.  ``P=0``: what ``gaussian_residual_stats`` needs; ``K=0`` (with ``P=0``): what
    ``gaussian_residuals`` needs, the factor scratch alone."""
    i32, i64 = C.c_int32, C.c_int64
    return _plan_query("gpz_gaussian_residual_plan", (B, D, Lt, K, P, nnz, slab_genes, perm_batch), slab_genes=i64, n_slabs=i64,
                       spot_slices=i32, factors_padded=i32, perm_batch=i32, batches=i64, partials_bytes=i64)


@dataclass(frozen=True)
class _ResidualFamily:
    """What differs between the count and the Gaussian residual entries, for ``_residual_model`` and ``_residual_run``."""
    params: tuple       # the model tensors after mean and scale, by the name the messages give them: an entry's head pointers
    shapes: object      # (Lt, B, D) -> their shapes
    elsewhere: str      # the refusal of sparse data on another device than the model's: .format(the data's, the model's)
    stored: object      # a whole sparse container -> (its pointers ahead of the rows' arrays, the SparseCounts that holds them)
    scalars: tuple      # the scalar arguments between Lt [, K] and slab_genes or the outputs, as keys of the checked arguments
    stems: dict         # stage -> the entry's name; data stored as its non-zeros goes to the entry of that name + "_sparse"
    plan: object        # (stage, B, G, Lt, K, P, nnz, slab_genes, perm_batch) -> the stage's plan


def _count_plan(stage, B, G, Lt, K, P, nnz, slab_genes, perm_batch):
    if stage in ("residuals", "morans_i"):
        return residual_autocorr_plan(B, G, Lt, nnz, 64 if stage == "residuals" else slab_genes)
    return residual_autocorr_perm_plan(B, G, Lt, K, P, nnz, slab_genes, perm_batch)


def _gaussian_plan(stage, B, G, Lt, K, P, nnz, slab_genes, perm_batch):
    return gaussian_residual_plan(B, G, Lt, K, P, nnz, slab_genes, perm_batch)


_COUNT_RESIDUALS = _ResidualFamily(
    params=("W", "V", "theta"), shapes=lambda Lt, B, D: ((D, Lt), (B,), (D,)),
    elsewhere="gpzoo_amd: the counts live on {}, the model on {}: move them with counts.to(device)",
    stored=lambda y: ([], y), scalars=("family", "kind", "lognormal"),
    stems=dict(residuals="gpz_count_residuals", morans_i="gpz_residual_morans_i", stats="gpz_residual_spatial_stats",
               perm="gpz_residual_autocorr_perm"),
    plan=_count_plan)
_GAUSSIAN_RESIDUALS = _ResidualFamily(
    params=("W", "b", "noise_sd"), shapes=lambda Lt, B, D: ((D, Lt), (D,), (D,)),
    elsewhere="gpzoo_amd: the expression lives on {}, the model on {}: move it with expr.to(device)",
    stored=lambda y: ([_ptr(y.offset)], y.values), scalars=("kind",),
    stems=dict(residuals="gpz_gaussian_residuals", stats="gpz_gaussian_residual_stats", perm="gpz_gaussian_residual_perm"),
    plan=_gaussian_plan)


def _residual_model(who, fam, sparse, mean, scale, y, params, genes):
    """What the residual entries of either family check before any device work, once the form of ``y`` and the kind are
    settled, and their arguments in the entries' types.  ``params``: the tensors of ``fam.params`` (None: an absent theta)."""
    if mean.dim() != 2:
        raise ValueError(f"{who}: mean must be (Lt, B), got shape {tuple(mean.shape)}")
    Lt, B = mean.shape
    D = y.shape[0]
    if (tuple(y.shape) != (D, B) or scale.shape != (Lt, B)
            or any(t is not None and t.shape != shape for t, shape in zip(params, fam.shapes(Lt, B, D)))):
        raise ValueError(f"{who}: y {tuple(y.shape)}, mean {tuple(mean.shape)}, scale {tuple(scale.shape)}, "
                         + ", ".join(f"{k} {tuple(t.shape)}" for k, t in zip(fam.params, params) if t is not None)
                         + " do not fit together")
    g = None
    if genes is not None:
        g = genes.detach() if isinstance(genes, torch.Tensor) else torch.as_tensor(genes)
        if g.dim() != 1 or g.numel() < 1 or g.is_floating_point() or g.dtype == torch.bool:
            raise ValueError(f"{who}: genes must be a non-empty 1-D list of gene indices")
        if bool(((g < 0) | (g >= D)).any()):
            raise IndexError(f"{who}: a gene index lies outside [0, {D})")
    dense = [mean, scale, *params, None if sparse else y]
    _need_cuda(*dense)
    dev = _same_device(*dense)
    if sparse and y.device != dev:
        raise RuntimeError(fam.elsewhere.format(y.device, dev))
    prep = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()  # noqa: E731
    if g is not None:
        g = g.to(device=dev, dtype=torch.int32).contiguous()
    return dict(zip(fam.params, map(prep, params)), mean=prep(mean), scale=prep(scale), y=y if sparse else prep(y), genes=g,
                sparse=sparse, dev=dev, B=B, D=D, G=D if g is None else int(g.numel()), Lt=Lt, nnz=y.nnz if sparse else 0)


def _residual_args(who, mean, scale, W_pos, V_pos, y, theta_pos, genes, kind, lognormal_mean):
    """Everything the residual entries check before any device work, and their arguments in the entries' types."""
    from .likelihoods import SparseCounts, TransposedCounts, _counts_expected
    if isinstance(y, TransposedCounts):
        raise TypeError(f"{who}: y is the .T (obs x feat) of a SparseCounts; pass the SparseCounts itself (genes x spots)")
    _counts_expected(y, who)
    sparse = isinstance(y, SparseCounts)
    if sparse:
        if y.base is not y:
            raise TypeError(f"{who}: a view y[:, idx]; the whole data set is needed")
    elif not isinstance(y, torch.Tensor):
        raise TypeError(f"{who}: y must be a dense (D, B) tensor or a whole SparseCounts, got {type(y).__name__}")
    if kind not in RESIDUAL_KINDS:
        raise ValueError(f'{who}: kind must be "pearson" or "deviance", got {kind!r}')
    a = _residual_model(who, _COUNT_RESIDUALS, sparse, mean, scale, y, (W_pos, V_pos, theta_pos), genes)
    return dict(a, family=int(theta_pos is not None), kind=RESIDUAL_KINDS[kind], lognormal=int(bool(lognormal_mean)))


def _gaussian_kind(who, kind):
    """The kinds of the Gaussian residuals; the deviance residual of a Gaussian is its Pearson residual."""
    if kind == "deviance":
        raise ValueError(f'{who}: kind="deviance" is kind="pearson" for a Gaussian -- the signed square root of the unit '
                         'deviance is (y - yhat) / noise_sd; ask for "pearson"')
    if kind not in GAUSSIAN_RESIDUAL_KINDS:
        raise ValueError(f'{who}: kind must be "pearson", "response" or "predictive", got {kind!r}')
    return GAUSSIAN_RESIDUAL_KINDS[kind]


def _gaussian_data(who, y):
    """The refusals of the data's form, which need no device; True for a whole ``SparseExpression``."""
    from .likelihoods import SparseCounts, SparseExpression, TransposedCounts
    if isinstance(y, (SparseCounts, TransposedCounts)):
        raise TypeError(f"{who}: a {type(y).__name__} holds counts; the Gaussian models take real-valued expression, a dense "
                        "(D, B) tensor or a whole SparseExpression")
    if isinstance(y, SparseExpression):
        if y.is_view:
            raise TypeError(f"{who}: a view y[:, idx]; the whole data set is needed")
        return True
    if not isinstance(y, torch.Tensor):
        raise TypeError(f"{who}: y must be a dense (D, B) tensor or a whole SparseExpression, got {type(y).__name__}")
    return False


def _gaussian_residual_args(who, mean, scale, W, b, noise_sd, y, genes, kind):
    """Everything the Gaussian residual entries check before any device work, and their arguments in the entries' types."""
    from .likelihoods import NOISE_SD_RANGE
    sparse = _gaussian_data(who, y)
    k = _gaussian_kind(who, kind)
    a = _residual_model(who, _GAUSSIAN_RESIDUALS, sparse, mean, scale, y, (W, b, noise_sd), genes)
    lo, hi = NOISE_SD_RANGE
    if not bool(((a["noise_sd"] >= lo) & (a["noise_sd"] <= hi)).all()):
        raise ValueError(f"{who}: noise_sd must lie in [{lo:g}, {hi:g}] (likelihoods.NOISE_SD_RANGE), positive and finite")
    return dict(a, kind=k)


def _residual_table(who, nbr, mean, slab_genes):
    """The checks ``residual_morans_i`` makes on its table and ``slab_genes`` before any device work; returns K."""
    if not isinstance(nbr, torch.Tensor) or nbr.dim() != 2 or nbr.dtype.is_floating_point or nbr.dtype == torch.bool:
        raise ValueError(f"{who}: nbr must be a (B, K) integer table")
    K = int(nbr.shape[1])
    if not 1 <= K <= 32:
        raise ValueError(f"{who}: K = {K} neighbours unsupported (1..32)")
    if int(slab_genes) != slab_genes or int(slab_genes) < 0 or int(slab_genes) % 64:
        raise ValueError(f"{who}: slab_genes = {slab_genes!r} is not a positive multiple of 64 (or 0: the plan's choice)")
    if nbr.shape[0] != mean.shape[-1]:
        raise ValueError(f"{who}: nbr {tuple(nbr.shape)} for {mean.shape[-1]} spots")
    if K >= nbr.shape[0]:
        raise ValueError(f"{who}: {K} neighbours of {nbr.shape[0]} spots (K < B needed)")
    return K


def _residual_perms(who, nbr, perms, perm_batch):
    """The checks the permutation entries make on ``perms`` and ``perm_batch`` before any device work."""
    _perm_table_check(who, perms, int(nbr.shape[0]), perm_batch)
    if perm_batch > 32:
        raise ValueError(f"{who}: perm_batch = {perm_batch} unsupported (0 = chosen by the plan, at most 32)")


_WIDE_KEYS = ("I", "C", "residual_mean", "residual_var", "kurtosis")


def _residual_run(fam, who, stage, a, nbr=None, K=0, slab_genes=0, perms=None, stat=0, perm_batch=0, return_sims=False):
    """One residual entry of the family ``fam`` on its checked arguments ``a``.  ``stage`` and what is returned: "residuals",
    the (B, G) fp32 array; "morans_i", [I, mean, variance]; "stats", [I, C, mean, variance, kurtosis]; "perm", [value, n_ge,
    n_le, sim_mean, sim_m2, sims or None, mean, variance, kurtosis].  A table or a permutation that the device refused raises
    ValueError (one synchronisation)."""
    lib = _lib.load()
    dev, B, G = a["dev"], a["B"], a["G"]
    tables = [] if nbr is None else [nbr.to(device=dev, dtype=torch.int64).contiguous()]
    if stage == "perm":
        tables.append(_perm_table(perms, B, dev))
    P = int(tables[1].shape[0]) if stage == "perm" else 0
    plan = fam.plan(stage, B, G, a["Lt"], K, P, a["nnz"], int(slab_genes), perm_batch)
    f64 = lambda n: [torch.empty(G, dtype=torch.float64, device=dev) for _ in range(n)]  # noqa: E731
    scalars = [a["Lt"], *(a[k] for k in fam.scalars)]
    if stage == "residuals":
        out = [torch.empty((B, G), dtype=torch.float32, device=dev)]
        outputs = [_ptr(out[0])]
    else:
        scalars[1:1] = [K]
        if stage == "perm":
            value, sim_mean, sim_m2, *moments = f64(6)
            n_ge, n_le = (torch.empty(G, dtype=torch.int32, device=dev) for _ in range(2))
            sims = torch.empty((G, P), dtype=torch.float64, device=dev) if return_sims else None
            out = [value, n_ge, n_le, sim_mean, sim_m2, sims, *moments]
            scalars += [int(slab_genes), P, stat, plan["perm_batch"]]
        else:
            out = f64(3 if stage == "morans_i" else 5)
            scalars += [int(slab_genes)]
        info = torch.empty(1, dtype=torch.int32, device=dev)
        outputs = [_ptr(t) for t in (*out, info)]
    if a["sparse"]:
        ahead, rows = fam.stored(a["y"])
        data = ahead + [_ptr(rows.row_ptr), _ptr(rows.row_spot), _ptr(rows.row_perm), _ptr(rows.col_val)]
        extents = [B, a["D"], a["nnz"], G]
    else:
        data, extents = [_ptr(a["y"])], [B, a["D"], G]
    entry = fam.stems[stage] + ("_sparse" if a["sparse"] else "")
    with torch.cuda.device(dev):
        ws = _workspace(dev, plan["partials_bytes"])
        rc = getattr(lib, entry)(*(_ptr(a[k]) for k in ("mean", "scale", *fam.params)), *data, _ptr(a["genes"]),
                                 *(_ptr(t) for t in tables), *extents, *scalars, *outputs, _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, entry)
    if stage == "residuals":
        return out[0]
    code = int(info.item())
    if code == 1 or (code != 0 and stage != "perm"):
        raise ValueError(f"{who}: the neighbour table has an entry outside [0, B) or naming its own row")
    if code != 0:
        raise ValueError(f"{who}: a row of perms is not a permutation of 0 .. B - 1 (an entry outside [0, B) or an index named twice)")
    return out


def _perm_result(stat, out):
    """(``AutocorrPerm``, moments) of the "perm" stage's outputs."""
    return AutocorrPerm(stat, *out[:6]), dict(zip(_WIDE_KEYS[2:], out[6:]))


def count_residuals(mean, scale, W_pos, V_pos, y, theta_pos=None, genes=None, kind="pearson", lognormal_mean: bool = True):
    """(B, G) fp32 residuals, spot-major, of the counts under the predictive mean rate mu = V W m of ``poisson_deviance``
    (gpz_count_residuals / gpz_count_residuals_sparse).  ``kind="pearson"``: (y - mu) / sqrt(mu (1 + mu / theta));
    ``"deviance"``: sign(y - mu) sqrt(unit deviance).  ``theta_pos`` (D,) selects the negative binomial, None the Poisson
    family.  ``genes``: a list of gene indices in any order, repeats allowed (column g is gene ``genes[g]``), or None for all.
    ``y``: dense (D, B), or a whole ``SparseCounts`` (the same bits as on its dense array)."""
    who = "count_residuals"
    a = _residual_args(who, mean, scale, W_pos, V_pos, y, theta_pos, genes, kind, lognormal_mean)
    return _residual_run(_COUNT_RESIDUALS, who, "residuals", a)


def residual_morans_i(mean, scale, W_pos, V_pos, y, nbr, theta_pos=None, genes=None, kind="pearson",
                      lognormal_mean: bool = True, slab_genes: int = 0) -> dict:
    """Moran's I of every gene's residuals (``count_residuals``' arguments) over the neighbour table nbr (B, K) int64 of
    distinct neighbours, 1 <= K <= 32, with weights 1 / K (gpz_residual_morans_i / gpz_residual_morans_i_sparse): a dict of
    fp64 (G,) tensors ``I``, ``residual_mean`` and ``residual_var`` (sum z^2 / B).  The genes are taken in slabs of
    ``slab_genes`` columns (0: ``residual_autocorr_plan``'s choice); neither the (D, B) rate nor the (D, B) residuals exist.
    Sums in a fixed order: repeated calls agree bit for bit.  A table entry outside [0, B) or naming its own row raises
    ValueError (checked on the device; one synchronisation)."""
    who = "residual_morans_i"
    K = _residual_table(who, nbr, mean, slab_genes)
    a = _residual_args(who, mean, scale, W_pos, V_pos, y, theta_pos, genes, kind, lognormal_mean)
    return dict(zip(("I", "residual_mean", "residual_var"), _residual_run(_COUNT_RESIDUALS, who, "morans_i", a, nbr, K, slab_genes)))


def residual_spatial_stats(mean, scale, W_pos, V_pos, y, nbr, theta_pos=None, genes=None, kind="pearson",
                           lognormal_mean: bool = True, slab_genes: int = 0) -> dict:
    """``residual_morans_i`` with Geary's C and the kurtosis beside I (gpz_residual_spatial_stats /
    gpz_residual_spatial_stats_sparse): a dict of fp64 (G,) tensors ``I``, ``C``, ``residual_mean``, ``residual_var`` and
    ``kurtosis`` (m4 / m2^2 of the residuals).  ``I``, ``residual_mean`` and ``residual_var`` are ``residual_morans_i``'s at
    the same ``slab_genes``, bit for bit.  A bad table raises ValueError (checked on the device; one synchronisation)."""
    who = "residual_spatial_stats"
    K = _residual_table(who, nbr, mean, slab_genes)
    a = _residual_args(who, mean, scale, W_pos, V_pos, y, theta_pos, genes, kind, lognormal_mean)
    return dict(zip(_WIDE_KEYS, _residual_run(_COUNT_RESIDUALS, who, "stats", a, nbr, K, slab_genes)))


def residual_autocorr_perm(mean, scale, W_pos, V_pos, y, nbr, perms, theta_pos=None, genes=None, kind="pearson",
                           lognormal_mean: bool = True, *, stat: str = "moran", return_sims: bool = False, perm_batch: int = 0,
                           slab_genes: int = 0):
    """Moran's I (``stat="moran"``) or Geary's C (``"geary"``) of every gene's residuals (``residual_morans_i``'s
    arguments) and of their P relabellings ``perms`` (P, B) integer, r^pi[n] = r[pi[n]], scored while each residual slab is
    resident (gpz_residual_autocorr_perm / gpz_residual_autocorr_perm_sparse): per slab the residuals are formed once, the
    observed statistics once, then every batch of ``perm_batch`` permutations (0: ``residual_autocorr_perm_plan``'s choice).
    Returns (``AutocorrPerm``, moments): ``value`` is ``residual_spatial_stats``' I or C, bit for bit; ``n_ge`` / ``n_le``
    compare the fp64 numerators (residuals are real-valued: a mathematical tie may fall either way in the last bit);
    ``sim_mean`` / ``sim_m2`` are folded in permutation order, so nothing depends on ``perm_batch``; ``sims`` (G, P) with
    ``return_sims``.  The moments are a dict of fp64 (G,) tensors ``residual_mean``, ``residual_var`` and ``kurtosis``.  A
    bad table and a row of ``perms`` that is no permutation raise ValueError (checked on the device; one synchronisation)."""
    who = "residual_autocorr_perm"
    st = _stat(who, stat)
    K = _residual_table(who, nbr, mean, slab_genes)
    _residual_perms(who, nbr, perms, perm_batch)
    a = _residual_args(who, mean, scale, W_pos, V_pos, y, theta_pos, genes, kind, lognormal_mean)
    return _perm_result(stat, _residual_run(_COUNT_RESIDUALS, who, "perm", a, nbr, K, slab_genes, perms, st, perm_batch, return_sims))


def gaussian_residuals(mean, scale, W, b, noise_sd, y, genes=None, kind="pearson"):
    """(B, G) fp32 residuals, spot-major, of real-valued expression under the Gaussian factor models' predictive mean
    yhat = b[:, None] + W mean (gpz_gaussian_residuals / gpz_gaussian_residuals_sparse).  ``kind="pearson"``:
    (y - yhat) / noise_sd; ``"response"``: y - yhat, in data units; ``"predictive"``: (y - yhat) / sqrt(v) with
    v = noise_sd^2 + W^2 scale^2, the standardisation that stays right where q(F) is wide.  ``"deviance"`` raises ValueError:
    for a Gaussian it is the Pearson residual.  ``genes`` as in ``count_residuals``.  ``y``: dense (D, B), or a whole
    ``SparseExpression`` (the same bits as on ``y.to_dense()``)."""
    who = "gaussian_residuals"
    a = _gaussian_residual_args(who, mean, scale, W, b, noise_sd, y, genes, kind)
    return _residual_run(_GAUSSIAN_RESIDUALS, who, "residuals", a)


def gaussian_residual_stats(mean, scale, W, b, noise_sd, y, nbr, genes=None, kind="pearson", slab_genes: int = 0) -> dict:
    """Moran's I, Geary's C and the moments of every gene's Gaussian residuals (``gaussian_residuals``' arguments) over the
    neighbour table nbr (B, K) (gpz_gaussian_residual_stats / gpz_gaussian_residual_stats_sparse): a dict of fp64 (G,) tensors
    ``I``, ``C``, ``residual_mean``, ``residual_var`` and ``kurtosis``, as ``residual_spatial_stats`` returns them.  I and C
    do not change under a per-gene affine map, so "pearson" and "response" give the same I and C up to fp32 rounding and
    differ in the moments; "predictive" differs spot by spot.  Neither the (D, B) mean nor the residuals exist: the genes are
    taken in slabs of ``slab_genes`` columns.  A bad table raises ValueError (checked on the device; one synchronisation)."""
    who = "gaussian_residual_stats"
    K = _residual_table(who, nbr, mean, slab_genes)
    a = _gaussian_residual_args(who, mean, scale, W, b, noise_sd, y, genes, kind)
    return dict(zip(_WIDE_KEYS, _residual_run(_GAUSSIAN_RESIDUALS, who, "stats", a, nbr, K, slab_genes)))


def gaussian_residual_autocorr_perm(mean, scale, W, b, noise_sd, y, nbr, perms, genes=None, kind="pearson", *, stat: str = "moran",
                                    return_sims: bool = False, perm_batch: int = 0, slab_genes: int = 0):
    """``residual_autocorr_perm`` for the Gaussian residuals (gpz_gaussian_residual_perm / gpz_gaussian_residual_perm_sparse):
    the observed I or C of every gene's residuals and of their P relabellings ``perms`` (P, B), scored while each residual
    slab is resident.  Returns (``AutocorrPerm``, moments) as there; ``value`` is ``gaussian_residual_stats``' I or C, bit for
    bit, and nothing depends on ``perm_batch``."""
    who = "gaussian_residual_autocorr_perm"
    st = _stat(who, stat)
    K = _residual_table(who, nbr, mean, slab_genes)
    _residual_perms(who, nbr, perms, perm_batch)
    a = _gaussian_residual_args(who, mean, scale, W, b, noise_sd, y, genes, kind)
    return _perm_result(stat, _residual_run(_GAUSSIAN_RESIDUALS, who, "perm", a, nbr, K, slab_genes, perms, st, perm_batch, return_sims))


def poisson_nsf_sparse_plan(N: int, B: int, D: int, Lt: int, E: int, nnz: int) -> dict:
    """How ``poisson_nsf_sparse`` covers a shape (gpz_poisson_nsf_sparse_plan, a host-only query: no device needed):
    ``gene_chunk`` (non-zeros of a gene row per wave of the gene pass), ``spot_chunk`` (the same for a spot's column; 0:
    columns are not split), ``n_gene_chunks`` (length of the gene pass's work list), ``samples_per_group`` (samples the spot
    pass holds on chip at a time), ``factors_padded`` (Lt rounded up to the kernel instance), ``workspace_bytes``."""
    lib = _lib.load()
    gc, sc, spg, fp, nch = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    rc = lib.gpz_poisson_nsf_sparse_plan(int(N), int(B), int(D), int(Lt), int(E), int(nnz), C.byref(gc), C.byref(sc),
                                         C.byref(nch), C.byref(spg), C.byref(fp))
    if rc != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return dict(gene_chunk=gc.value, spot_chunk=sc.value, n_gene_chunks=nch.value, samples_per_group=spg.value,
                factors_padded=fp.value,
                workspace_bytes=int(lib.gpz_poisson_nsf_sparse_workspace_bytes(int(N), int(B), int(D), int(nnz), int(Lt), int(E))))


@_on_device
def poisson_nsf_sparse(mean, scale, eps, W_pos, V_pos, counts, idx=None, with_lgamma: bool = True):
    """``poisson_nsf`` for counts held as their non-zeros (gpz_poisson_nsf_sparse): the same 5-tuple
    (loglik fp64 scalar, dmean, dscale, dW, dV), as exact sums over the non-zeros -- O(nnz E Lt + E Lt B + D Lt) work.

    counts: a ``likelihoods.SparseCounts`` (D, N), or the view ``counts[:, idx]`` of one.  mean, scale (Lt,B); eps (E,Lt,B);
    W_pos (D,Lt); V_pos (B,) with B = N, or B = len(idx) for a view.  ``idx``: shorthand for ``counts[:, idx]``.
    Any number of samples goes through one call.  Nothing here waits for the device: the call can be captured in a graph."""
    from .likelihoods import SparseCounts
    if not isinstance(counts, SparseCounts):
        raise TypeError(f"poisson_nsf_sparse: counts must be a SparseCounts, got {type(counts).__name__}")
    if idx is not None:
        counts = counts[:, idx]
    _need_cuda(mean, scale, eps, W_pos, V_pos)
    dev = mean.device
    if counts.device != dev:
        raise RuntimeError(f"gpzoo_amd: the counts live on {counts.device}, the model on {dev}: move them with counts.to(device)")
    lib = _lib.load()
    f32 = torch.float32
    mean, scale = mean.detach().to(f32).contiguous(), scale.detach().to(f32).contiguous()
    eps = eps.detach().to(f32).contiguous()
    W_pos, V_pos = W_pos.detach().to(f32).contiguous(), V_pos.detach().to(f32).contiguous()
    if W_pos.data_ptr() % 16:
        W_pos = W_pos.clone()            # the entry reads rows of W 16 bytes at a time (include/gpzoo_hip.h)
    base = counts.base
    D, N = base.shape
    Lt, B = mean.shape
    E = eps.shape[0]
    if counts.shape != (W_pos.shape[0], B) or scale.shape != (Lt, B) or eps.shape != (E, Lt, B) or \
            W_pos.shape != (D, Lt) or V_pos.shape != (B,):
        raise ValueError(f"poisson_nsf_sparse: counts {tuple(counts.shape)}, mean {tuple(mean.shape)}, scale {tuple(scale.shape)}, "
                         f"eps {tuple(eps.shape)}, W {tuple(W_pos.shape)}, V {tuple(V_pos.shape)} do not fit together")
    ll = torch.empty(2, dtype=torch.float64, device=dev)
    dmean, dscale = torch.empty((Lt, B), dtype=f32, device=dev), torch.empty((Lt, B), dtype=f32, device=dev)
    dW, dV = torch.empty((D, Lt), dtype=f32, device=dev), torch.empty((B,), dtype=f32, device=dev)
    nbytes = lib.gpz_poisson_nsf_sparse_workspace_bytes(N, B, D, base.nnz, Lt, E)
    if nbytes == 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    ws = _workspace(dev, nbytes)
    rc = lib.gpz_poisson_nsf_sparse(_ptr(mean), _ptr(scale), _ptr(eps), _ptr(W_pos), _ptr(V_pos), _ptr(base.col_ptr),
                                    _ptr(base.col_gene), _ptr(base.col_val), _ptr(base.row_ptr), _ptr(base.row_spot),
                                    _ptr(base.row_perm), _ptr(counts.idx), _ptr(counts.pos), N, B, D, base.nnz, Lt, E,
                                    int(with_lgamma), _ptr(ll), _ptr(dmean), _ptr(dscale), _ptr(dW), _ptr(dV), _ptr(ws),
                                    ws.numel(), _stream(dev))
    _lib.check(rc, "gpz_poisson_nsf_sparse")
    total = ll[0] - ll[1] if with_lgamma else ll[0].clone()
    return total, dmean, dscale, dW, dV


def nb_nsf_sparse_plan(N: int, B: int, D: int, Lt: int, E: int, nnz: int) -> dict:
    """How ``nb_nsf_sparse`` covers a shape (gpz_nb_nsf_sparse_plan, a host-only query: no device needed): ``gene_chunk``
    (non-zeros of a gene row per wave of the gene pass), ``n_gene_chunks`` (length of its work list), ``factors_padded`` and
    ``zero_factors_padded`` (Lt rounded up to the kernel instance of the non-zero and of the zero passes), ``gene_slices`` and
    ``spot_slices`` (partial slabs of the zero part's two passes), ``samples_per_group`` and ``zero_samples_per_group``
    (samples held on chip at a time), ``samples_per_call`` (more are split on the host; the other entries describe the
    first call), ``workspace_bytes``."""
    lib = _lib.load()
    ee = min(int(E), 32)
    gc, nch = C.c_int32(), C.c_int64()
    fp, zfp, gsl, ssl, spg, zspg = (C.c_int32() for _ in range(6))
    rc = lib.gpz_nb_nsf_sparse_plan(int(N), int(B), int(D), int(Lt), ee, int(nnz), C.byref(gc), C.byref(nch), C.byref(fp),
                                    C.byref(zfp), C.byref(gsl), C.byref(ssl), C.byref(spg), C.byref(zspg))
    if rc != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return dict(gene_chunk=gc.value, n_gene_chunks=nch.value, factors_padded=fp.value, zero_factors_padded=zfp.value,
                gene_slices=gsl.value, spot_slices=ssl.value, samples_per_group=spg.value,
                zero_samples_per_group=zspg.value, samples_per_call=ee,
                workspace_bytes=int(lib.gpz_nb_nsf_sparse_workspace_bytes(int(N), int(B), int(D), int(nnz), int(Lt), ee)))


@_on_device
def nb_nsf_sparse(mean, scale, eps, W_pos, V_pos, theta_pos, counts, idx=None, with_lgamma: bool = True):
    """``nb_nsf`` for counts held as their non-zeros (gpz_nb_nsf_sparse): the same 6-tuple
    (loglik fp64 scalar, dmean, dscale, dW, dV, dtheta).  -theta log1p(mu / theta) needs no counts and is a dense pass over the
    batch; everything that carries a factor y is a sum over the non-zeros.  Nothing of D x B elements exists.

    counts: a ``likelihoods.SparseCounts`` (D, N), or the view ``counts[:, idx]`` of one.  mean, scale (Lt,B); eps (E,Lt,B);
    W_pos (D,Lt); theta_pos (D,); V_pos (B,) with B = N, or B = len(idx) for a view.  ``idx``: shorthand for ``counts[:, idx]``.
    Up to 32 samples go through one call; more are split as in ``nb_nsf`` (the sample-independent terms count once).
    Nothing here waits for the device: the call can be captured in a graph."""
    from .likelihoods import SparseCounts
    if not isinstance(counts, SparseCounts):
        raise TypeError(f"nb_nsf_sparse: counts must be a SparseCounts, got {type(counts).__name__}")
    if idx is not None:
        counts = counts[:, idx]
    _need_cuda(mean, scale, eps, W_pos, V_pos, theta_pos)
    dev = mean.device
    if counts.device != dev:
        raise RuntimeError(f"gpzoo_amd: the counts live on {counts.device}, the model on {dev}: move them with counts.to(device)")
    lib = _lib.load()
    f32 = torch.float32
    mean, scale, eps, W_pos, V_pos, theta_pos = (t.detach().to(f32).contiguous()
                                                 for t in (mean, scale, eps, W_pos, V_pos, theta_pos))
    # the entry wants 16-byte aligned arrays (include/gpzoo_hip.h); a contiguous view keeps its storage offset
    mean, scale, eps, W_pos, V_pos, theta_pos = (t if t.data_ptr() % 16 == 0 else t.clone()
                                                 for t in (mean, scale, eps, W_pos, V_pos, theta_pos))
    base = counts.base
    D, N = base.shape
    if mean.dim() != 2 or eps.dim() != 3:
        raise ValueError(f"nb_nsf_sparse: mean {tuple(mean.shape)} must be (Lt, B) and eps {tuple(eps.shape)} (E, Lt, B)")
    Lt, B = mean.shape
    E = eps.shape[0]
    if counts.shape != (W_pos.shape[0], B) or scale.shape != (Lt, B) or eps.shape != (E, Lt, B) or \
            W_pos.shape != (D, Lt) or V_pos.shape != (B,) or theta_pos.shape != (D,):
        raise ValueError(f"nb_nsf_sparse: counts {tuple(counts.shape)}, mean {tuple(mean.shape)}, scale {tuple(scale.shape)}, "
                         f"eps {tuple(eps.shape)}, W {tuple(W_pos.shape)}, V {tuple(V_pos.shape)}, theta {tuple(theta_pos.shape)} "
                         "do not fit together")
    eg = 32                                  # samples per call (NMAXE of csrc/nb_sparse.hip)
    total = torch.zeros((), dtype=torch.float64, device=dev)
    shapes = ((Lt, B), (Lt, B), (D, Lt), (B,), (D,))
    acc = [torch.zeros(s, dtype=f32, device=dev) for s in shapes] if E > eg else None
    for e0 in range(0, E, eg):
        ee = min(eg, E - e0)
        ll = torch.empty(2, dtype=torch.float64, device=dev)
        out = [torch.empty(s, dtype=f32, device=dev) for s in shapes]
        nbytes = lib.gpz_nb_nsf_sparse_workspace_bytes(N, B, D, base.nnz, Lt, ee)
        if nbytes == 0:
            raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
        ws = _workspace(dev, nbytes)
        rc = lib.gpz_nb_nsf_sparse(_ptr(mean), _ptr(scale), _ptr(eps[e0:e0 + ee]), _ptr(W_pos), _ptr(V_pos), _ptr(theta_pos),
                                   _ptr(base.col_ptr), _ptr(base.col_gene), _ptr(base.col_val), _ptr(base.row_ptr),
                                   _ptr(base.row_spot), _ptr(base.row_perm), _ptr(counts.idx), _ptr(counts.pos), N, B, D,
                                   base.nnz, Lt, ee, int(with_lgamma and e0 == 0), _ptr(ll), _ptr(out[0]), _ptr(out[1]),
                                   _ptr(out[2]), _ptr(out[3]), _ptr(out[4]), _ptr(ws), ws.numel(), _stream(dev))
        _lib.check(rc, "gpz_nb_nsf_sparse")
        if E <= eg:                          # one call: its outputs are the result
            total = ll[0] - ll[1] if with_lgamma else ll[0].clone()
            return (total, *out)
        wgt = ee / E
        # loglik[0] and dtheta carry the sample-independent terms in full in every part: the weights sum to one
        total += wgt * ll[0]
        if with_lgamma and e0 == 0:
            total -= ll[1]          # the parameter-free lgamma(y+1) term is evaluated once
        for a_, o_ in zip(acc, out):
            a_.add_(o_, alpha=wgt)
    return (total, *acc)


def _deviance_result(per_gene, per_spot, null_per_gene, scalars):
    return dict(per_gene=per_gene, per_spot=per_spot, null_per_gene=null_per_gene, total=scalars[0], sum_y=scalars[1],
                sum_mu=scalars[2], null_total=scalars[3])


def poisson_deviance_plan(N: int, D: int, Lt: int) -> dict:
    """How ``poisson_deviance`` covers a shape (gpz_poisson_deviance_plan, a host-only query: no device needed):
    ``spots_per_tile`` x ``genes_per_tile`` (one wave's tile), ``genes_per_block`` (one workgroup's genes = one per-spot
    partial slab), ``gene_slices`` (number of those), ``spot_slices`` (per-gene partial slabs) of ``tiles_per_spot_slice``
    tiles each, ``factors_padded``, ``workspace_bytes``."""
    lib = _lib.load()
    v = [C.c_int32() for _ in range(5)]
    tper, fp = C.c_int64(), C.c_int32()
    rc = lib.gpz_poisson_deviance_plan(int(N), int(D), int(Lt), *(C.byref(x) for x in v), C.byref(tper), C.byref(fp))
    if rc != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return dict(spots_per_tile=v[0].value, genes_per_tile=v[1].value, genes_per_block=v[2].value, gene_slices=v[3].value,
                spot_slices=v[4].value, tiles_per_spot_slice=tper.value, factors_padded=fp.value,
                workspace_bytes=int(lib.gpz_poisson_deviance_workspace_bytes(int(N), int(D), int(Lt))))


def poisson_deviance_sparse_plan(N: int, B: int, D: int, Lt: int, nnz: int) -> dict:
    """The same for ``poisson_deviance_sparse`` (gpz_poisson_deviance_sparse_plan): ``gene_chunk`` (non-zeros of a gene row
    per wave), ``spot_chunk`` (0: columns are not split), ``n_gene_chunks``, ``factors_padded``, ``workspace_bytes``."""
    lib = _lib.load()
    gc, sc, fp, nch = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    rc = lib.gpz_poisson_deviance_sparse_plan(int(N), int(B), int(D), int(Lt), int(nnz), C.byref(gc), C.byref(sc),
                                              C.byref(nch), C.byref(fp))
    if rc != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return dict(gene_chunk=gc.value, spot_chunk=sc.value, n_gene_chunks=nch.value, factors_padded=fp.value,
                workspace_bytes=int(lib.gpz_poisson_deviance_sparse_workspace_bytes(int(N), int(B), int(D), int(nnz), int(Lt))))


@_on_device
def poisson_deviance(mean, scale, W_pos, V_pos, y, lognormal_mean: bool = True):
    """Poisson deviance of the counts under the predictive mean rate (gpz_poisson_deviance): mu = V W m with
    m = exp(mean + scale^2 / 2) (``lognormal_mean``; exp(mean) without) and dev = 2 (y log(y / mu) - y + mu), 2 mu at y = 0.

    mean, scale (Lt,N); W_pos (D,Lt) and V_pos (N,) positive; y (D,N), read once; the (D,N) rate is never materialised.
    Returns a dict of fp64 tensors without a graph: ``per_gene`` (D,), ``per_spot`` (N,), ``null_per_gene`` (D,) -- the
    deviance of one constant rate per gene given V -- and the 0-d ``total``, ``sum_y``, ``sum_mu``, ``null_total``.
    Nothing here waits for the device."""
    _need_cuda(mean, scale, W_pos, V_pos, y)
    lib = _lib.load()
    f32 = torch.float32
    mean, scale = mean.detach().to(f32).contiguous(), scale.detach().to(f32).contiguous()
    W_pos, V_pos, y = W_pos.detach().to(f32).contiguous(), V_pos.detach().to(f32).contiguous(), y.detach().to(f32).contiguous()
    if W_pos.data_ptr() % 16:
        W_pos = W_pos.clone()            # the entry wants W 16-byte aligned (include/gpzoo_hip.h)
    Lt, N = mean.shape
    D = y.shape[0]
    if y.shape != (D, N) or scale.shape != (Lt, N) or W_pos.shape != (D, Lt) or V_pos.shape != (N,):
        raise ValueError(f"poisson_deviance: y {tuple(y.shape)}, mean {tuple(mean.shape)}, scale {tuple(scale.shape)}, "
                         f"W {tuple(W_pos.shape)}, V {tuple(V_pos.shape)} do not fit together")
    dev = mean.device
    f64 = torch.float64
    per_gene, null_per_gene = torch.empty(D, dtype=f64, device=dev), torch.empty(D, dtype=f64, device=dev)
    per_spot, scalars = torch.empty(N, dtype=f64, device=dev), torch.empty(4, dtype=f64, device=dev)
    nbytes = lib.gpz_poisson_deviance_workspace_bytes(N, D, Lt)
    if nbytes == 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    ws = _workspace(dev, nbytes)
    rc = lib.gpz_poisson_deviance(_ptr(mean), _ptr(scale), _ptr(W_pos), _ptr(V_pos), _ptr(y), N, D, Lt, int(bool(lognormal_mean)),
                                  _ptr(per_gene), _ptr(per_spot), _ptr(null_per_gene), _ptr(scalars), _ptr(ws), ws.numel(),
                                  _stream(dev))
    _lib.check(rc, "gpz_poisson_deviance")
    return _deviance_result(per_gene, per_spot, null_per_gene, scalars)


@_on_device
def poisson_deviance_sparse(mean, scale, W_pos, V_pos, counts, idx=None, lognormal_mean: bool = True):
    """``poisson_deviance`` for counts held as their non-zeros (gpz_poisson_deviance_sparse): the same dict, as exact sums
    over the stored values plus O((D + B) Lt) dense terms.

    counts: a ``likelihoods.SparseCounts`` (D, N), or the view ``counts[:, idx]`` of one.  mean, scale (Lt,B); W_pos (D,Lt);
    V_pos (B,) with B = N, or B = len(idx) for a view; ``per_spot`` follows the view's order.  ``idx``: shorthand for
    ``counts[:, idx]`` (its validation is deferred inside ``deferred_info()``).  Nothing here waits for the device."""
    from .likelihoods import SparseCounts
    if not isinstance(counts, SparseCounts):
        raise TypeError(f"poisson_deviance_sparse: counts must be a SparseCounts, got {type(counts).__name__}")
    if idx is not None:
        counts = counts[:, idx]
    _need_cuda(mean, scale, W_pos, V_pos)
    dev = mean.device
    if counts.device != dev:
        raise RuntimeError(f"gpzoo_amd: the counts live on {counts.device}, the model on {dev}: move them with counts.to(device)")
    lib = _lib.load()
    f32 = torch.float32
    mean, scale = mean.detach().to(f32).contiguous(), scale.detach().to(f32).contiguous()
    W_pos, V_pos = W_pos.detach().to(f32).contiguous(), V_pos.detach().to(f32).contiguous()
    if W_pos.data_ptr() % 16:
        W_pos = W_pos.clone()
    base = counts.base
    D, N = base.shape
    Lt, B = mean.shape
    if counts.shape != (W_pos.shape[0], B) or scale.shape != (Lt, B) or W_pos.shape != (D, Lt) or V_pos.shape != (B,):
        raise ValueError(f"poisson_deviance_sparse: counts {tuple(counts.shape)}, mean {tuple(mean.shape)}, "
                         f"scale {tuple(scale.shape)}, W {tuple(W_pos.shape)}, V {tuple(V_pos.shape)} do not fit together")
    f64 = torch.float64
    per_gene, null_per_gene = torch.empty(D, dtype=f64, device=dev), torch.empty(D, dtype=f64, device=dev)
    per_spot, scalars = torch.empty(B, dtype=f64, device=dev), torch.empty(4, dtype=f64, device=dev)
    nbytes = lib.gpz_poisson_deviance_sparse_workspace_bytes(N, B, D, base.nnz, Lt)
    if nbytes == 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    ws = _workspace(dev, nbytes)
    rc = lib.gpz_poisson_deviance_sparse(_ptr(mean), _ptr(scale), _ptr(W_pos), _ptr(V_pos), _ptr(base.col_ptr),
                                         _ptr(base.col_gene), _ptr(base.col_val), _ptr(base.row_ptr), _ptr(base.row_spot),
                                         _ptr(base.row_perm), _ptr(counts.idx), _ptr(counts.pos), N, B, D, base.nnz, Lt,
                                         int(bool(lognormal_mean)), _ptr(per_gene), _ptr(per_spot), _ptr(null_per_gene),
                                         _ptr(scalars), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, "gpz_poisson_deviance_sparse")
    return _deviance_result(per_gene, per_spot, null_per_gene, scalars)


def _nb_deviance_result(per_gene, per_spot, null_per_gene, ll_gene, ll_spot, pll_gene, scalars):
    return dict(per_gene=per_gene, per_spot=per_spot, null_per_gene=null_per_gene, loglik_per_gene=ll_gene,
                loglik_per_spot=ll_spot, poisson_loglik_per_gene=pll_gene, total=scalars[0], sum_y=scalars[1],
                sum_mu=scalars[2], null_total=scalars[3], loglik=scalars[4], poisson_loglik=scalars[5])


def nb_deviance_plan(N: int, D: int, Lt: int) -> dict:
    """How ``nb_deviance`` covers a shape (gpz_nb_deviance_plan, a host-only query: no device needed); the keys of
    ``poisson_deviance_plan``."""
    lib = _lib.load()
    v = [C.c_int32() for _ in range(5)]
    tper, fp = C.c_int64(), C.c_int32()
    rc = lib.gpz_nb_deviance_plan(int(N), int(D), int(Lt), *(C.byref(x) for x in v), C.byref(tper), C.byref(fp))
    if rc != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return dict(spots_per_tile=v[0].value, genes_per_tile=v[1].value, genes_per_block=v[2].value, gene_slices=v[3].value,
                spot_slices=v[4].value, tiles_per_spot_slice=tper.value, factors_padded=fp.value,
                workspace_bytes=int(lib.gpz_nb_deviance_workspace_bytes(int(N), int(D), int(Lt))))


def nb_deviance_sparse_plan(N: int, B: int, D: int, Lt: int, nnz: int) -> dict:
    """The same for ``nb_deviance_sparse`` (gpz_nb_deviance_sparse_plan); the keys of ``poisson_deviance_sparse_plan``."""
    lib = _lib.load()
    gc, sc, fp, nch = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    rc = lib.gpz_nb_deviance_sparse_plan(int(N), int(B), int(D), int(Lt), int(nnz), C.byref(gc), C.byref(sc), C.byref(nch),
                                         C.byref(fp))
    if rc != 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    return dict(gene_chunk=gc.value, spot_chunk=sc.value, n_gene_chunks=nch.value, factors_padded=fp.value,
                workspace_bytes=int(lib.gpz_nb_deviance_sparse_workspace_bytes(int(N), int(B), int(D), int(nnz), int(Lt))))


def _nb_deviance_outputs(D, B, dev):
    f64 = torch.float64
    return [torch.empty(n, dtype=f64, device=dev) for n in (D, B, D, D, B, D, 6)]


@_on_device
def nb_deviance(mean, scale, W_pos, V_pos, theta_pos, y, lognormal_mean: bool = True):
    """Negative-binomial scoring of the counts under the predictive mean rate (gpz_nb_deviance): mu as in
    ``poisson_deviance``, one inverse dispersion ``theta_pos`` (D,) > 0 per gene;
    dev = 2 [y log(y / mu) - (y + theta) log1p((y - mu) / (mu + theta))], ll = log NB(y | mu, theta), pll = log Poisson(y | mu).

    Returns a dict of fp64 tensors without a graph: ``per_gene``, ``null_per_gene``, ``loglik_per_gene``,
    ``poisson_loglik_per_gene`` (D,), ``per_spot``, ``loglik_per_spot`` (N,) and the 0-d ``total``, ``sum_y``, ``sum_mu``,
    ``null_total``, ``loglik``, ``poisson_loglik``.  The null model has the Poisson null's rate per gene and the gene's own
    theta.  y is read twice; the (D,N) rate is never materialised.  Nothing here waits for the device."""
    _need_cuda(mean, scale, W_pos, V_pos, theta_pos, y)
    lib = _lib.load()
    f32 = torch.float32
    mean, scale = mean.detach().to(f32).contiguous(), scale.detach().to(f32).contiguous()
    W_pos, V_pos, y = W_pos.detach().to(f32).contiguous(), V_pos.detach().to(f32).contiguous(), y.detach().to(f32).contiguous()
    theta_pos = theta_pos.detach().to(f32).contiguous()
    if W_pos.data_ptr() % 16:
        W_pos = W_pos.clone()            # the entry wants W 16-byte aligned (include/gpzoo_hip.h)
    Lt, N = mean.shape
    D = y.shape[0]
    if (y.shape != (D, N) or scale.shape != (Lt, N) or W_pos.shape != (D, Lt) or V_pos.shape != (N,)
            or theta_pos.shape != (D,)):
        raise ValueError(f"nb_deviance: y {tuple(y.shape)}, mean {tuple(mean.shape)}, scale {tuple(scale.shape)}, "
                         f"W {tuple(W_pos.shape)}, V {tuple(V_pos.shape)}, theta {tuple(theta_pos.shape)} do not fit together")
    dev = mean.device
    outs = _nb_deviance_outputs(D, N, dev)
    nbytes = lib.gpz_nb_deviance_workspace_bytes(N, D, Lt)
    if nbytes == 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    ws = _workspace(dev, nbytes)
    rc = lib.gpz_nb_deviance(_ptr(mean), _ptr(scale), _ptr(W_pos), _ptr(V_pos), _ptr(theta_pos), _ptr(y), N, D, Lt,
                             int(bool(lognormal_mean)), *(_ptr(o) for o in outs), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, "gpz_nb_deviance")
    return _nb_deviance_result(*outs)


@_on_device
def nb_deviance_sparse(mean, scale, W_pos, V_pos, theta_pos, counts, idx=None, lognormal_mean: bool = True):
    """``nb_deviance`` for counts held as their non-zeros (gpz_nb_deviance_sparse): the same dict, as one dense pass over the
    batch that reads no counts plus sums over the stored values.

    counts: a ``likelihoods.SparseCounts`` (D, N), or the view ``counts[:, idx]`` of one.  mean, scale (Lt,B); W_pos (D,Lt);
    V_pos (B,); theta_pos (D,); the per-spot outputs follow the view's order.  ``idx``: shorthand for ``counts[:, idx]``.
    Nothing here waits for the device."""
    from .likelihoods import SparseCounts
    if not isinstance(counts, SparseCounts):
        raise TypeError(f"nb_deviance_sparse: counts must be a SparseCounts, got {type(counts).__name__}")
    if idx is not None:
        counts = counts[:, idx]
    _need_cuda(mean, scale, W_pos, V_pos, theta_pos)
    dev = mean.device
    if counts.device != dev:
        raise RuntimeError(f"gpzoo_amd: the counts live on {counts.device}, the model on {dev}: move them with counts.to(device)")
    lib = _lib.load()
    f32 = torch.float32
    mean, scale = mean.detach().to(f32).contiguous(), scale.detach().to(f32).contiguous()
    W_pos, V_pos = W_pos.detach().to(f32).contiguous(), V_pos.detach().to(f32).contiguous()
    theta_pos = theta_pos.detach().to(f32).contiguous()
    if W_pos.data_ptr() % 16:
        W_pos = W_pos.clone()
    base = counts.base
    D, N = base.shape
    Lt, B = mean.shape
    if (counts.shape != (W_pos.shape[0], B) or scale.shape != (Lt, B) or W_pos.shape != (D, Lt) or V_pos.shape != (B,)
            or theta_pos.shape != (D,)):
        raise ValueError(f"nb_deviance_sparse: counts {tuple(counts.shape)}, mean {tuple(mean.shape)}, "
                         f"scale {tuple(scale.shape)}, W {tuple(W_pos.shape)}, V {tuple(V_pos.shape)}, "
                         f"theta {tuple(theta_pos.shape)} do not fit together")
    outs = _nb_deviance_outputs(D, B, dev)
    nbytes = lib.gpz_nb_deviance_sparse_workspace_bytes(N, B, D, base.nnz, Lt)
    if nbytes == 0:
        raise ValueError(lib.gpz_last_error().decode("utf-8", "replace"))
    ws = _workspace(dev, nbytes)
    rc = lib.gpz_nb_deviance_sparse(_ptr(mean), _ptr(scale), _ptr(W_pos), _ptr(V_pos), _ptr(theta_pos), _ptr(base.col_ptr),
                                    _ptr(base.col_gene), _ptr(base.col_val), _ptr(base.row_ptr), _ptr(base.row_spot),
                                    _ptr(base.row_perm), _ptr(counts.idx), _ptr(counts.pos), N, B, D, base.nnz, Lt,
                                    int(bool(lognormal_mean)), *(_ptr(o) for o in outs), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, "gpz_nb_deviance_sparse")
    return _nb_deviance_result(*outs)


def profile_enable(on: bool = True):
    _lib.check(_lib.load().gpz_profile_enable(int(on)), "gpz_profile_enable")


def profile_read() -> dict:
    n = len(_lib.PROF_SLOTS)
    ms = (C.c_double * n)()
    cnt = (C.c_int32 * n)()
    _lib.check(_lib.load().gpz_profile_read(ms, cnt, n), "gpz_profile_read")
    return {name: (ms[i], cnt[i]) for i, name in enumerate(_lib.PROF_SLOTS) if not name.startswith("_")}
