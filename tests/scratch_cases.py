"""One row per library entry and variant that carves scratch memory (TEST INFRASTRUCTURE ONLY; importable without a GPU:
tests/test_scratch_cases.py checks the table on the CPU, tests/test_hip_scratch.py runs it on the GPU).

gpzoo_amd/ops.py keeps one scratch buffer per (device, stream); every entry carves its plan out of it and nothing clears
it between calls, and every output is a ``torch.empty``.  A row runs one entry through ``ops`` at a SMALL shape -- one
slice in every sliced dimension, every extent off its tile multiple -- and at a LARGE one -- at least two slices, the last
one short, in every count the entry's plan reports -- so that the GPU test can run SMALL on the bytes LARGE left behind,
on 0xFF and on 0x40, and ask for the same bits each time ("Scratch and output initialisation").

Inputs and oracles are the project's own case modules (poisson_cases, nb_cases, sparse_poisson_cases, sparse_nb_cases,
deviance_cases, nb_deviance_cases, nmf_oracle, kmeans_cases, kmeans_oracle, entry_cases, spatial_oracle, smooth_oracle, the
SVGP oracle and gpzoo_amd.synthetic, the problem generator of tests/test_hip_wide.py); the tolerances are the ones the
entry's own GPU test file uses, named at each ``check``.  No tolerance is introduced here.  Every row has a ``check``; the
VNNGP rows that pass g_kl and g_chol check their forward outputs only (their gradients are held to equal bits).

A Row has
  name      the pytest id
  entries   the ``gpz_*`` functions of include/gpzoo_hip.h the row runs (tests/test_scratch_cases.py: every entry that takes
            a workspace is in some row)
  shapes    {"small": ..., "large": ...}, with the derivation of LARGE beside it
  build     which -> dict of CPU inputs (cached; tensors are never modified)
  prepare   inputs -> device state (default: every tensor moved to the GPU)
  run       (ops, state) -> dict of output tensors; opaque byte buffers are not returned, their consumer's outputs are
  slices    which -> dict of the slice counts of the plan (1 each for SMALL, >= 2 each for LARGE), or None
  bytes     which -> workspace bytes of the first call, or None (no host-only query for the entry)
  check     (which, inputs, out) -> None; asserts against the fp64 oracle at the entry's own tolerance, or None
  index     {output name: (inputs -> exclusive upper bound)} of the outputs that are indices
  dtype     the floating type the entry runs in (inputs must be exactly representable in it)"""
from __future__ import annotations

import ctypes as C
import functools
import itertools
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np
import torch

import deviance_cases as DC
import entry_cases as EC
import kmeans_cases as KC
import kmeans_oracle as KO
import nb_cases as NBC
import nb_deviance_cases as NDC
import nmf_oracle as NO
import poisson_cases as PC
import sparse_nb_cases as SNC
import sparse_poisson_cases as SPC

F32, F64 = torch.float32, torch.float64
WHICH = ("small", "large")


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def _to_cuda(inputs: dict) -> dict:
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in inputs.items()}


@dataclass
class Row:
    name: str
    entries: tuple
    shapes: dict
    build: Callable
    run: Callable
    dtype: torch.dtype = F32
    prepare: Callable = _to_cuda
    slices: Optional[Callable] = None
    bytes: Optional[Callable] = None
    check: Optional[Callable] = None
    index: dict = field(default_factory=dict)

    def inputs(self, which: str) -> dict:
        return _inputs(self.name, which)


ROWS: list = []
_BY_NAME: dict = {}


def add(row: Row) -> Row:
    assert row.name not in _BY_NAME, row.name
    ROWS.append(row)
    _BY_NAME[row.name] = row
    return row


def row(name: str) -> Row:
    return _BY_NAME[name]


@functools.lru_cache(maxsize=None)
def _inputs(name: str, which: str) -> dict:
    r = _BY_NAME[name]
    return r.build(which)


def _lib():
    from gpzoo_amd import _lib as L
    return L


def _code(dtype) -> int:
    return _lib().GPZ_F32 if dtype == F32 else _lib().GPZ_F64


def _gen(*seed) -> torch.Generator:
    return torch.Generator().manual_seed(int(sum(s * 1009 ** i for i, s in enumerate(seed))) % (2 ** 31))


def _randn(g, *s, dtype=F32):
    return torch.randn(*s, generator=g, dtype=F64).to(dtype)


def _rand(g, *s, dtype=F32):
    return torch.rand(*s, generator=g, dtype=F64).to(dtype)


def _close(got, ref, tol, what):
    err = (got.detach().double().cpu() - ref).abs()
    worst = float((err / tol).max()) if err.numel() else 0.0
    print(what, "err/tol", f"{worst:.3g}")
    assert bool(torch.isfinite(got).all()) and worst <= 1.0, (what, worst)


# =====================================================================================================================
# kernel-matrix gradient: gpz_kgrad (csrc/kgrad.hip).  Scratch: the fp64 accumulator of (L,4) + (nA,4) partial sums,
# cleared by a memset, added to by every 256-column trip.  LARGE: nB = 513 is three trips with a one-column last trip
# (entry_cases.kgrad_plan), nA = 1025 is five 256-row finish blocks with a one-row last block.
# =====================================================================================================================

def _kgrad_build(dtype, which, shapes):
    nA, nB = shapes[which]
    c = EC.kernel_case("rbf", 2, nA, nB, L=3, seed=1)
    c["Kbar"] = EC.upstreams(c)["dense"]
    c["run_dtype"] = dtype
    return c


def _kgrad_run(ops, s):
    dt = s["run_dtype"]
    spec = ops.KernelSpec(EC.KIND_ID["rbf"], s["sigma"].to(dt), s["ell"].to(dt), True)
    gth, gpt = ops.kgrad(spec, s["A"].to(dt), s["B"].to(dt), s["Kbar"].to(dt))
    return dict(grad_theta=gth, grad_A=gpt)


def _kgrad_check(dtype):
    def check(which, c, out):
        ref = EC.kernel_grads(c, c["Kbar"])          # tests/test_hip_kernel_grads.py::_close, entry_cases.grad_tol
        _close(out["grad_theta"], ref["theta"], EC.grad_tol(ref["theta"], dtype), f"kgrad {which} theta")
        _close(out["grad_A"], ref["A"], EC.grad_tol(ref["A"], dtype), f"kgrad {which} A")
    return check


for _dt, _nm in ((F32, "f32"), (F64, "f64")):
    _sh = dict(small=(5, 70), large=(1025, 513))
    add(Row(f"kgrad-{_nm}", ("gpz_kgrad",), _sh, functools.partial(_kgrad_build, _dt, shapes=_sh), _kgrad_run, _dt,
            bytes=lambda w, sh=_sh: _lib().load().gpz_kgrad_workspace_bytes(sh[w][0], 3), check=_kgrad_check(_dt),
            slices=lambda w, sh=_sh: dict(column_trips=EC.cdiv(sh[w][1], 256), finish_blocks=EC.cdiv(sh[w][0], 256))))


# =====================================================================================================================
# factorisation and triangular solve: gpz_potrf_batched, gpz_trsm_lln_batched (csrc/factor.hip, coop.hip).  Scratch: the
# padded copy, Dinv and the one-launch path's ticket and flag words.  LARGE: M = 300 is three 128-blocks, padded by 84;
# the right-hand side of 130 columns is two 128-column blocks, padded.  The path is the library's choice (one launch at
# these orders: gpz_factor_path); the launch-per-step path is chosen once per process by GPZ_FACTOR_PATH and runs in a
# child process (tests/test_hip_scratch.py::test_launch_per_step_factorisation).
# =====================================================================================================================

def _spd(batch, M, seed, dtype):
    g = _gen(seed, M)
    A = torch.randn(batch, M, M + 8, generator=g, dtype=F64)
    return (A @ A.transpose(-1, -2) / M + 0.5 * torch.eye(M, dtype=F64)).to(dtype)      # tests/test_hip_linalg.py::spd


def _factor_build(dtype, which, shapes):
    M, N = shapes[which]
    A = _spd(2, M, 7, dtype)
    return dict(A=A, B=_randn(_gen(M, N), 2, M, N, dtype=dtype))


def _factor_run(ops, s):
    Lc = ops.cholesky(s["A"])
    return dict(chol=Lc, solve=ops.solve_triangular_lower(Lc, s["B"]))


def _factor_check(dtype):
    def check(which, c, out):
        ref = torch.linalg.cholesky(c["A"].double())
        got = out["chol"].double().cpu()
        Lg = out["chol"].cpu()
        refX = torch.linalg.solve_triangular(Lg.double(), c["B"].double(), upper=False)
        if dtype == F64:      # tests/test_hip_linalg.py: test_cholesky_matches_lapack, test_trsm_matches_lapack
            torch.testing.assert_close(got, ref, rtol=1e-9, atol=1e-11)
            torch.testing.assert_close(out["solve"].cpu(), refX, rtol=1e-8, atol=1e-10)
        else:                 # test_fp32_storage_factor_entries
            torch.testing.assert_close(got, ref, rtol=2e-7, atol=2e-7)
            torch.testing.assert_close(out["solve"].double().cpu(), refX, rtol=1e-6, atol=1e-6 * float(refX.abs().max()))
        assert torch.equal(got.triu(1), torch.zeros_like(got))
    return check


FACTOR_SHAPES = dict(small=(70, 37), large=(300, 130))
for _dt, _nm in ((F64, "f64"), (F32, "f32")):
    add(Row(f"factor-{_nm}", ("gpz_potrf_batched", "gpz_trsm_lln_batched"), FACTOR_SHAPES,
            functools.partial(_factor_build, _dt, shapes=FACTOR_SHAPES), _factor_run, _dt, check=_factor_check(_dt),
            bytes=lambda w: _lib().load().gpz_potrf_workspace_bytes(FACTOR_SHAPES[w][0], 2),
            slices=lambda w: dict(row_blocks=cdiv(FACTOR_SHAPES[w][0], 128), rhs_blocks=cdiv(FACTOR_SHAPES[w][1], 128))))


# =====================================================================================================================
# SVGP forward and backward: gpz_svgp_forward, gpz_svgp_backward (csrc/svgp.hip).  Problems from gpzoo_amd.synthetic (the
# generator of tests/test_hip_wide.py): configuration 3 (Matern-3/2, d = 2).  SMALL (N, M, L) = (777, 100, 2): one
# 128-block of inducing points (padded by 28), one chunk of columns, N no multiple of 128.  LARGE = (2000, 384, 3) on the
# tile paths -- three row blocks -- and (2000, 300, 3), padded by 84, on the panel path and in fp64; with chunk = 896 (seven
# 128-column tiles) the 777 columns of SMALL are one chunk and the 2000 of LARGE three, the last of 208.
# out["path"]: bit 0 = wide tiles, bit 1 = generated Kzx, 4 = the panel kernel.  2 alone needs the generated operand without
# the wide tile kernel: the narrow flag wins over it (0), and wide_product_supported fails only from Mp nc 4 >= 2^31 bytes
# on, at no shape a test can afford.  The rows cover 0, 1, 3 and 4.
# =====================================================================================================================

def _svgp_build(dtype, which, shapes, cfg=3):
    from gpzoo_amd.synthetic import make_config
    N, M, L = shapes[which]
    c = make_config(cfg, N=N, M=M, L=L, dtype=dtype)
    g = _gen(N, M, L)
    c["g_mean"], c["g_scale"] = _randn(g, L, N, dtype=dtype), _randn(g, L, N, dtype=dtype)
    c["g_kl"] = _randn(g, L, dtype=F64)
    c["g_chol"] = (0.01 * _randn(g, L, M, M, dtype=dtype)).tril()
    return c


def _svgp_prepare(c):
    from gpzoo_amd.configs import spec_for_config
    s = _to_cuda(c)
    s["spec"], s["extra"] = spec_for_config(s, torch.device("cuda", 0))
    return s


def _fwd(ops, s, whitened, **kw):
    return ops.svgp_forward(s["spec"], s["X"], s["Z"], s["mu"], s["Lu_raw"], s["jitter"], whitened, y=s["y"],
                            noise_sd=s["noise_sd"], **s["extra"], **kw)


FWD_OUT = ("mean", "scale", "Lu", "kl", "loglik", "elbo", "info")


def _bwd(ops, s, whitened, fwd, chunk=0, **kw):
    return ops.svgp_backward(s["spec"], s["X"], s["Z"], s["mu"], s["Lu_raw"], s["jitter"], whitened, s["g_mean"], s["g_scale"],
                             fwd["scale"], chunk=chunk, **s["extra"], **kw)


def _host_problem(c: dict, whitened: bool, keep: list, **kw):
    """The gpz_svgp_problem ``ops.svgp_forward(**kw)`` fills for the case, on host tensors: enough for the host-only
    path and workspace queries."""
    from gpzoo_amd import ops
    L = _lib()
    spec = ops.KernelSpec(L.KERNEL_MATERN32, c["sigma"].reshape(-1), c["lengthscale"].reshape(-1), True)
    p, _ = ops._problem(spec, c["X"], c["Z"], c["mu"], c["Lu_raw"], c["jitter"], whitened, None, None, 1e-6, keep)
    keep.append(torch.zeros(spec.L, dtype=torch.int32))
    p.info = keep[-1].data_ptr()
    if kw.get("materialize_kzx") is not None:
        p.flags |= L.SVGP_MATERIALIZE_KZX if kw["materialize_kzx"] else L.SVGP_GENERATE_KZX
    if kw.get("narrow_tiles"):
        p.flags |= L.SVGP_NARROW_TILES
    if kw.get("panel_products"):
        p.flags |= L.SVGP_PANEL_PRODUCTS
    return p


def svgp_forward_path(c: dict, whitened: bool, chunk: int = 0, **kw) -> int:
    """gpz_svgp_forward_path of the case under the flags ``ops.svgp_forward`` sets for ``kw`` (host only)."""
    keep: list = []
    return int(_lib().load().gpz_svgp_forward_path(C.byref(_host_problem(c, whitened, keep, **kw)), int(chunk)))


def _fwd_check(whitened, elbo=True, prefixes=("",)):
    """``elbo=False``: the row passes no observations (the moments do not depend on them); ``prefixes``: the row returns
    the outputs of several forward calls under these prefixes, each checked."""
    def check(which, c, out):
        for pre in prefixes:
            _check({k[len(pre):]: v for k, v in out.items() if k.startswith(pre)}, c)

    def _check(out, c):
        # tests/test_hip_wide.py::test_each_path_against_the_oracle (fp32), helpers.rtol_for per precision
        from helpers import rtol_for
        from oracle import svgp_oracle as O
        import pytest
        c64 = {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in c.items()}
        e, mean, scale = O.elbo_eval(c["kind"], whitened, c64["X"], c64["y"], c64["Z"], c64["sigma"], c64["lengthscale"],
                                     c64["mu"], c64["Lu_raw"], c["jitter"], c["noise_sd"])
        rt = rtol_for(c["dtype"])
        torch.testing.assert_close(out["mean"].double().cpu(), mean, rtol=rt, atol=rt * float(mean.abs().max()))
        torch.testing.assert_close(out["scale"].double().cpu(), scale, rtol=rt, atol=0)
        if elbo:
            assert float(out["elbo"]) == pytest.approx(float(e), rel=rt)
    return check


SVGP_TILE = dict(small=(777, 100, 2), large=(2000, 384, 3))
SVGP_PAD = dict(small=(777, 100, 2), large=(2000, 300, 3))
SVGP_CHUNK = 896

# (name, dtype, whitened, shapes, forward keywords, path reported)
FORWARD_VARIANTS = [
    ("path0", F32, True, SVGP_TILE, dict(materialize_kzx=True, narrow_tiles=True), 0),
    ("path1", F32, True, SVGP_TILE, dict(materialize_kzx=True), 1),
    ("path0-generate_refused", F32, True, SVGP_TILE, dict(materialize_kzx=False, narrow_tiles=True), 0),
    ("path3", F32, True, SVGP_TILE, dict(materialize_kzx=False), 3),
    ("path4", F32, True, SVGP_PAD, dict(panel_products=True), 4),
    ("f32-unwhitened", F32, False, SVGP_PAD, dict(), None),
    ("f64-whitened", F64, True, SVGP_PAD, dict(), 0),
    ("f64-unwhitened", F64, False, SVGP_PAD, dict(), 0),
    ("f32-chunks", F32, True, SVGP_PAD, dict(chunk=SVGP_CHUNK), None),
    ("path4-chunks", F32, True, SVGP_PAD, dict(panel_products=True, chunk=SVGP_CHUNK), 4),
    ("f64-chunks", F64, False, SVGP_PAD, dict(chunk=SVGP_CHUNK), 0),
]


def _svgp_slices(shapes, chunk):
    def slices(which):
        N, M, _ = shapes[which]
        out = dict(row_blocks=cdiv(M, 128))
        if chunk:
            out["column_chunks"] = cdiv(N, chunk)
        return out
    return slices


def _svgp_bytes(dtype, whitened, shapes, chunk=0, backward=False, **kw):
    def nbytes(which):
        keep: list = []
        p = _host_problem(_inputs_of_svgp(dtype, which, shapes), whitened, keep, **kw)
        lib = _lib().load()
        fn = lib.gpz_svgp_backward_workspace_bytes if backward else lib.gpz_svgp_workspace_bytes
        return int(fn(C.byref(p), int(chunk)))
    return nbytes


@functools.lru_cache(maxsize=None)
def _svgp_cached(dtype, which, shape):
    return _svgp_build(dtype, which, {which: shape})


def _inputs_of_svgp(dtype, which, shapes):
    return _svgp_cached(dtype, which, shapes[which])


for _nm, _dt, _wh, _sh, _kw, _path in FORWARD_VARIANTS:
    def _run(ops, s, wh=_wh, kw=_kw, path=_path):
        o = _fwd(ops, s, wh, **kw)
        assert path is None or o["path"] == path, (o["path"], path)
        return {k: o[k] for k in FWD_OUT}
    add(Row(f"svgp_forward-{_nm}", ("gpz_svgp_forward",), _sh, functools.partial(_inputs_of_svgp, _dt, shapes=_sh), _run, _dt,
            prepare=_svgp_prepare, check=_fwd_check(_wh), slices=_svgp_slices(_sh, _kw.get("chunk", 0)),
            bytes=_svgp_bytes(_dt, _wh, _sh, **_kw)))


def _fwd_no_y_run(ops, s):
    """Without observations the pass has no likelihood term: loglik and elbo are still written (scal is a torch.empty),
    and so is chol when asked for."""
    o = ops.svgp_forward(s["spec"], s["X"], s["Z"], s["mu"], s["Lu_raw"], s["jitter"], True, want_chol=True, **s["extra"])
    return {k: o[k] for k in FWD_OUT + ("chol",)}


add(Row("svgp_forward-no_y-chol", ("gpz_svgp_forward",), SVGP_PAD, functools.partial(_inputs_of_svgp, F32, shapes=SVGP_PAD),
        _fwd_no_y_run, F32, prepare=_svgp_prepare, slices=_svgp_slices(SVGP_PAD, 0), check=_fwd_check(True, elbo=False)))


def _fwd_retain_run(ops, s, chunk=0):
    """retain_wt: the written extent of wt_cache ([: L Mp ncp] words per chunk slot, as tests/test_hip_wide.py compares it)
    for the unchunked call, and the backward pass that consumes the buffer."""
    o = _fwd(ops, s, True, retain_wt=0.9, want_Lu=False, chunk=chunk)
    assert "wt_cache" in o
    L, M, N = s["L"], s["M"], s["N"]
    out = {k: o[k] for k in FWD_OUT if k in o}
    if not chunk:
        nwt = L * cdiv(M, 128) * 128 * cdiv(N, 128) * 128
        out["wt_written"] = o["wt_cache"].view(torch.int32)[:nwt].clone()
    gm, gl = _bwd(ops, s, True, o, chunk=chunk, wt_cache=o["wt_cache"])
    out.update(grad_mu=gm, grad_Lu=gl)
    return out


def _fwd_cache_run(ops, s, whitened=True):
    """A factor cache, invalid at the first call (the factor is built into a fresh ``torch.empty``) and valid at the
    second; the backward pass then takes the factor and the q(U) operands from it."""
    cache = ops.FactorCache()
    a = _fwd(ops, s, whitened, cache=cache)
    b = _fwd(ops, s, whitened, cache=cache)
    out = {f"first_{k}": a[k] for k in FWD_OUT}
    out.update({f"second_{k}": b[k] for k in FWD_OUT})
    gm, gl = _bwd(ops, s, whitened, b, cache=cache)
    out.update(grad_mu=gm, grad_Lu=gl)
    return out


for _nm, _fn, _dt, _sh in (("retain_wt", _fwd_retain_run, F32, SVGP_TILE),
                           ("retain_wt-chunks", functools.partial(_fwd_retain_run, chunk=SVGP_CHUNK), F32, SVGP_PAD),
                           ("factor_cache-f32", _fwd_cache_run, F32, SVGP_PAD),
                           ("factor_cache-f64-unwhitened", functools.partial(_fwd_cache_run, whitened=False), F64, SVGP_PAD)):
    add(Row(f"svgp_forward-{_nm}", ("gpz_svgp_forward", "gpz_svgp_backward"), _sh,
            functools.partial(_inputs_of_svgp, _dt, shapes=_sh), _fn, _dt, prepare=_svgp_prepare,
            check=_fwd_check("unwhitened" not in _nm, prefixes=("first_", "second_") if "cache" in _nm else ("",)),
            slices=_svgp_slices(_sh, SVGP_CHUNK if "chunks" in _nm else 0)))


@functools.lru_cache(maxsize=None)
def _bwd_case(which, whitened):
    """backward_forms_cases.make_case at the row's shape with its dense upstream (gm, gs, w, gc): what
    tests/test_hip_backward_forms.py runs, so that ``oracle_grads`` is the reference."""
    import backward_forms_cases as BC
    N, M, L = SVGP_PAD[which]
    c = BC.make_case(N, M, L)
    c.update(BC.make_upstream(c, whitened, "dense"))
    return c


def _bwd_build(dtype, whitened, which):
    return dict(_bwd_case(which, whitened), run_dtype=dtype)


def _bwd_prepare(c):
    from gpzoo_amd import _lib as L, ops
    dt = c["run_dtype"]
    s = {k: (v.to(dt).cuda() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in c.items()}
    s["w"] = c["w"].cuda()
    s["spec"] = ops.KernelSpec(L.KERNEL_RBF, s["sigma"], s["lengthscale"], True)
    return s


def _bwd_run(ops, s, whitened, form, narrow, kgrads, wt, chunk):
    a = (s["spec"], s["X"], s["Z"], s["mu"], s["Lu_raw"], s["jitter"], whitened)
    o = ops.svgp_forward(*a, want_Lu=False, retain_wt=0.9 if wt else 0.0, clamp_min=s["clamp_min"], chunk=chunk)
    assert ("wt_cache" in o) == wt
    res = ops.svgp_backward(*a, s["gm"], s["gs"], o["scale"], kernel_grads=kgrads, g_chol=s["gc"] if kgrads else None,
                            g_kl=s["w"], narrow_tiles=narrow, form=form, wt_cache=o.get("wt_cache"), clamp_min=s["clamp_min"],
                            chunk=chunk)
    out = dict(mu=res[0], Lu_raw=res[1])
    if kgrads:
        out.update(sigma=res[2][:, 0], lengthscale=res[2][:, 1], Z=res[3])
    return out


def _bwd_check(dtype, whitened):
    def check(which, c, out):
        # tests/test_hip_backward_forms.py::_check_against_oracle: fp64 1e-6, fp32 CEIL32 by whitened (or four times the
        # deviation of the oracle's own fp32 evaluation), against fp64 autograd of backward_forms_cases.oracle_grads
        import backward_forms_cases as BC
        import test_hip_backward_forms as TB
        ref = BC.oracle_grads(c, whitened, "dense")
        ref32 = lambda: BC.oracle_grads(c, whitened, "dense", dtype=F32)      # noqa: E731
        TB._check_against_oracle({k: v.double().cpu() for k, v in out.items()}, ref, dtype == F32, whitened,
                                 f"scratch {which}", ref32)
    return check


# every form x tile kernel x kernel gradients x retained Wt x precision; fp64 runs un-whitened (the other algebra), the
# chunked variants cover the per-chunk partial sums (mu_part, any_d, the Wt slots)
for _form, _narrow, _kg, _wt, _dt in itertools.product(("classic", "algebra"), (False, True), (False, True), (False, True),
                                                       (F32, F64)):
    _wh = _dt == F32
    _chunk = SVGP_CHUNK if (_kg != _wt) else 0
    _nm = "svgp_backward-{}-{}-{}-{}-{}{}".format(_form, "narrow" if _narrow else "wide", "all" if _kg else "qu",
                                                  "wt" if _wt else "nowt", "f32" if _dt == F32 else "f64-unwhitened",
                                                  "-chunks" if _chunk else "")
    add(Row(_nm, ("gpz_svgp_backward", "gpz_svgp_forward"), SVGP_PAD, functools.partial(_bwd_build, _dt, _wh),
            functools.partial(_bwd_run, whitened=_wh, form=_form, narrow=_narrow, kgrads=_kg, wt=_wt, chunk=_chunk), _dt,
            prepare=_bwd_prepare, check=_bwd_check(_dt, _wh), slices=_svgp_slices(SVGP_PAD, _chunk),
            bytes=_svgp_bytes(_dt, _wh, SVGP_PAD, _chunk, backward=True)))


# =====================================================================================================================
# precomputed W: gpz_wsvgp_precomputed, gpz_wsvgp_precomputed_backward (csrc/svgp.hip pre_carve, pre_carve_bwd).
# entry_cases.precomputed_case; LARGE (L, N, M) = (2, 1300, 300): three row blocks, N and M padded.
# =====================================================================================================================

PRE_SHAPES = dict(small=(2, 129, 33), large=(2, 1300, 300))


def _pre_build(dtype, which):
    c = EC.precomputed_case(*PRE_SHAPES[which])
    c["run_dtype"] = dtype
    return c


def _pre_run(ops, s):
    dt = s["run_dtype"]
    W, sig, mu, Lu = (s[k].to(dt) for k in ("W", "sigma", "mu", "Lu_raw"))
    o = ops.wsvgp_precomputed(W, sig, mu, Lu)
    gm, gl, gs = ops.wsvgp_precomputed_backward(W, sig, mu, Lu, s["R1"].to(dt), s["R2"].to(dt), o["scale"])
    return dict(mean=o["mean"], scale=o["scale"], Lu=o["Lu"], grad_mu=gm, grad_Lu=gl, grad_sigma=gs)


def _pre_check(dtype):
    def check(which, c, out):
        ref = EC.precomputed_ref(c)                  # tests/test_hip_precomputed.py through entry_cases.pre_tol
        for k in ("mean", "scale", "Lu", "grad_mu", "grad_Lu", "grad_sigma"):
            _close(out[k], ref[k], EC.pre_tol(ref[k], dtype, relative_only=(k == "scale")) + 1e-300, f"precomputed {which} {k}")
    return check


for _dt, _nm in ((F32, "f32"), (F64, "f64")):
    add(Row(f"wsvgp_precomputed-{_nm}", ("gpz_wsvgp_precomputed", "gpz_wsvgp_precomputed_backward"), PRE_SHAPES,
            functools.partial(_pre_build, _dt), _pre_run, _dt, check=_pre_check(_dt),
            slices=lambda w: dict(row_blocks=cdiv(PRE_SHAPES[w][2], 128)),
            bytes=lambda w, dt=_dt: _lib().load().gpz_wsvgp_precomputed_workspace_bytes(*PRE_SHAPES[w], _code(dt))))


# =====================================================================================================================
# VNNGP: gpz_vnngp_forward, gpz_vnngp_backward (csrc/vnngp.hip).  LARGE (N, M, L) = (1030, 300, 3): three row blocks of the
# factorisation, padded; K = 8 neighbours.  The backward pass builds its inverted index (inv, istart, itmp, ihist, idup)
# in scratch; with a point_order the records are laid out through idxp / Xp.
# =====================================================================================================================

VNN_SHAPES = dict(small=(70, 20, 2), large=(1030, 300, 3))
VNN_K = 8


def _vnn_build(dtype, which):
    c = _svgp_build(dtype, which, VNN_SHAPES, cfg=2)
    c["Lu_raw"] = c["Lu_raw"].to(dtype)
    return c


def _vnn_prepare(c):
    from gpzoo_amd import ops
    s = _svgp_prepare(c)
    s["order"] = ops.morton_order(s["X"])
    return s


def _vnn_run(ops, s, full):
    a = (s["spec"], s["X"], s["Z"], s["mu"], s["Lu_raw"], s["jitter"], VNN_K)
    o = ops.vnngp_forward(*a, keep_state=full)
    out = {k: o[k] for k in ("mean", "scale", "Lu", "chol", "kl", "idx")}
    if full:
        res = ops.vnngp_backward(*a, o["idx"], s["g_mean"], s["g_scale"], kernel_grads=True, g_chol=s["g_chol"], g_kl=s["g_kl"],
                                 state=o["state"], point_order=s["order"])
    else:
        res = ops.vnngp_backward(*a, o["idx"], s["g_mean"], s["g_scale"])
    out.update(zip(("grad_mu", "grad_Lu", "grad_theta", "grad_Z"), res))
    return out


def _vnn_check(dtype, full):
    def check(which, c, out):
        # tests/test_hip_vnngp.py::test_caller_table_with_repeated_neighbours: rt = 1e-7 (fp64) / 2e-3 (fp32); mean and
        # gradients rtol rt with atol rt max|ref|, scale atol rt 1e-2; torch autograd over the oracle on the same table.
        # The rows with g_kl and g_chol check the forward only: that file has no reference for their sum.
        from oracle import svgp_oracle as O
        leaf = {k: c[k].double().clone().requires_grad_(not full and k in ("mu", "Lu_raw")) for k in ("Z", "sigma",
                "lengthscale", "mu", "Lu_raw")}
        sig, ell = leaf["sigma"].reshape(-1), leaf["lengthscale"].reshape(-1)
        mean, scale, _, _, _ = O.vnngp_moments(c["X"].double(), leaf["Z"], sig, ell, leaf["mu"], leaf["Lu_raw"], c["jitter"], VNN_K,
                                               idx=out["idx"].cpu())
        rt = 1e-7 if dtype == F64 else 2e-3
        torch.testing.assert_close(out["mean"].double().cpu(), mean.detach(), rtol=rt, atol=rt * float(mean.abs().max()))
        torch.testing.assert_close(out["scale"].double().cpu(), scale.detach(), rtol=rt, atol=rt * 1e-2)
        if not full:
            ((c["g_mean"].double() * mean).sum() + (c["g_scale"].double() * scale).sum()).backward()
            for k, nm in (("mu", "grad_mu"), ("Lu_raw", "grad_Lu")):
                ref = leaf[k].grad
                torch.testing.assert_close(out[nm].double().cpu(), ref, rtol=rt, atol=rt * float(ref.abs().max()))
    return check


for _dt, _full in itertools.product((F32, F64), (False, True)):
    add(Row("vnngp-{}-{}".format("f32" if _dt == F32 else "f64", "state-grads-order" if _full else "plain"),
            ("gpz_vnngp_forward", "gpz_vnngp_backward", "gpz_knn"), VNN_SHAPES, functools.partial(_vnn_build, _dt),
            functools.partial(_vnn_run, full=_full), _dt, prepare=_vnn_prepare, check=_vnn_check(_dt, _full),
            slices=lambda w: dict(row_blocks=cdiv(VNN_SHAPES[w][1], 128)), index=dict(idx=lambda c: c["M"])))


# =====================================================================================================================
# spatial graph and Moran's I: gpz_spatial_knn, gpz_morans_i (csrc/spatial.hip).  sk_plan: T = ceil(N / 64) tiles and
# S = ceil(T / 64) boxes of tiles, so LARGE N = 4200 is 66 tiles (the last of 40 points) in 2 boxes (the last of 2 tiles).
# An order brings the ``seen`` / ``bad`` words into play; ops.spatial_knn always passes one, the C entry takes none too.
# Moran's I: partial sums per 256 rows, LARGE N = 1030 is five (the last of 6 rows).
# =====================================================================================================================

SK_SHAPES = dict(small=(50,), large=(4200,))
SK_K = 6


def _sk_build(which):
    (N,) = SK_SHAPES[which]
    return dict(X=_rand(_gen(N, 5), N, 2, dtype=F32) * 100.0, N=N)


def _sk_run(ops, s, order):
    if order:
        return dict(idx=ops.spatial_knn(s["X"], SK_K))
    lib = _lib().load()
    X, N = s["X"], s["N"]
    idx = ops.torch.empty((N, SK_K), dtype=torch.int64, device=X.device)      # ops' torch: poisoned with its other outputs
    ws = ops._workspace(X.device, lib.gpz_spatial_knn_workspace_bytes(N, 2, SK_K))
    rc = lib.gpz_spatial_knn(ops._ptr(X), N, 2, SK_K, _lib().GPZ_F32, None, ops._ptr(idx), ops._ptr(ws), ws.numel(),
                             ops._stream(X.device))
    _lib().check(rc, "gpz_spatial_knn")
    return dict(idx=idx)


def _sk_check(which, c, out):
    import spatial_oracle as SO                     # tests/test_hip_spatial_autocorr.py::test_graph_equals_oracle: exact
    rows = np.arange(c["N"]) if c["N"] <= 4099 else np.random.default_rng(1).choice(c["N"], 1024, replace=False)
    np.testing.assert_array_equal(out["idx"].cpu().numpy()[rows], SO.knn_rows(c["X"].numpy(), SK_K, rows))


for _order in (True, False):
    add(Row("spatial_knn-{}".format("order" if _order else "no_order"), ("gpz_spatial_knn",), SK_SHAPES, _sk_build,
            functools.partial(_sk_run, order=_order), F32, index=dict(idx=lambda c: c["N"]), check=_sk_check,
            bytes=lambda w: _lib().load().gpz_spatial_knn_workspace_bytes(SK_SHAPES[w][0], 2, SK_K),
            slices=lambda w: dict(tiles=cdiv(SK_SHAPES[w][0], 64), boxes=cdiv(cdiv(SK_SHAPES[w][0], 64), 64))))

MI_SHAPES = dict(small=(70, 3), large=(1030, 5))


def _mi_build(which):
    N, L = MI_SHAPES[which]
    nbr = (torch.arange(N)[:, None] + 1 + 7 * torch.arange(SK_K)[None, :]) % N        # a ring graph: never the own row
    return dict(values=_randn(_gen(N, L), N, L, dtype=F32), nbr=nbr.to(torch.int64))


def _mi_check(which, c, out):
    import spatial_oracle as SO                     # tests/test_hip_spatial_autocorr.py::test_morans_i_matches_oracle_...
    want = SO.morans_i(c["values"].double().numpy(), c["nbr"].numpy())
    np.testing.assert_allclose(out["I"].cpu().numpy(), want, rtol=0, atol=1e-10)


add(Row("morans_i", ("gpz_morans_i",), MI_SHAPES, _mi_build, lambda ops, s: dict(I=ops.morans_i(s["values"], s["nbr"])), F32,
        check=_mi_check,
        bytes=lambda w: _lib().load().gpz_morans_i_workspace_bytes(*MI_SHAPES[w], SK_K),
        slices=lambda w: dict(row_chunks=cdiv(MI_SHAPES[w][0], 256))))


# =====================================================================================================================
# kNN regression: gpz_knn_mean (csrc/smooth.hip).  Scratch: the fp64 copies of X and Z only, written in full by km_stage
# before the search reads them.  LARGE (N, M, K, L) = (3000, 300, 17, 5): more than one workgroup of queries.
# =====================================================================================================================

KM_SHAPES = dict(small=(70, 20, 5, 3), large=(3000, 300, 17, 5))


def _knn_mean_build(which):
    N, M, K, L = KM_SHAPES[which]
    g = _gen(N, M, K)
    # factors in [1, 2): same-sign sums, so the relative bound of the oracle comparison is meaningful for every mean
    return dict(X=_rand(g, N, 2, dtype=F32), F=_rand(g, N, L, dtype=F32) + 1.0, Z=_rand(g, M, 2, dtype=F32), K=K, N=N)


def _knn_mean_run(ops, s):
    U, idx = ops.knn_mean(s["X"], s["F"], s["Z"], s["K"], return_index=True)
    return dict(U=U, idx=idx)


def _knn_mean_check(which, c, out):
    import smooth_oracle as SM                      # tests/test_hip_smooth_factors.py::test_index_sets_equal_the_oracle
    want_U, want = SM.knn_mean(c["X"].numpy(), c["F"].numpy(), c["Z"].numpy(), c["K"], np.arange(c["Z"].shape[0]))
    np.testing.assert_array_equal(out["idx"].cpu().numpy(), want)
    np.testing.assert_allclose(out["U"].cpu().numpy(), want_U, rtol=1e-12, atol=0)


add(Row("knn_mean", ("gpz_knn_mean",), KM_SHAPES, _knn_mean_build, _knn_mean_run, F32, index=dict(idx=lambda c: c["N"]),
        check=_knn_mean_check,
        bytes=lambda w: _lib().load().gpz_knn_mean_workspace_bytes(KM_SHAPES[w][0], KM_SHAPES[w][1], 2, KM_SHAPES[w][2],
                                                                   KM_SHAPES[w][3]),
        slices=lambda w: dict(query_blocks=cdiv(KM_SHAPES[w][1], 256))))


# =====================================================================================================================
# k-means: gpz_kmeans_seed, gpz_kmeans_lloyd, gpz_kmeans_assign (csrc/kmeans.hip).  kmeans_cases.split_plan restates the
# launch arithmetic: LARGE (N, M) = (5000, 300) is 20 point tiles (the last of 136 points), two centre tiles (the last
# of 44) and two splits; the seeding's block totals are 20 as well.
# =====================================================================================================================

KMEANS_SHAPES = dict(small=(70, 5), large=(5000, 300))


def _kmeans_build(which):
    N, M = KMEANS_SHAPES[which]
    X, C0 = KC.random_case(N, M, 2, "f32", seed=4)
    u = np.random.default_rng([N, M]).random((M, KO.n_trials(M)))
    return dict(X=torch.from_numpy(X), C0=torch.from_numpy(C0), u=torch.from_numpy(u), N=N, M=M)


def _kmeans_seed_run(ops, s):
    idx, Cs = ops.kmeans_seed(s["X"], s["M"], s["u"])
    return dict(idx=idx, C=Cs)


def _kmeans_lloyd_run(ops, s):
    Cc = s["C0"].clone()
    labels = torch.full((s["N"],), -1, dtype=torch.int32, device=Cc.device)
    state = ops.kmeans_state(Cc.device)
    ops.kmeans_lloyd(s["X"], Cc, labels, state, 0.0, 3)
    return dict(C=Cc, labels=labels, state=state)


def _kmeans_assign_run(ops, s):
    labels, inertia, d2 = ops.kmeans_assign(s["X"], s["C0"], return_d2=True)
    return dict(labels=labels, inertia=inertia, d2=d2)


def _kmeans_slices(w):
    p = KC.split_plan(*KMEANS_SHAPES[w])
    return dict(point_tiles=p["tiles"], centre_tiles=p["ctiles"], splits=p["splits"])


def _kmeans_check(nm):
    def check(which, c, out):
        X, C0, u = c["X"].numpy(), c["C0"].numpy(), c["u"].numpy()
        if nm == "seed":          # tests/test_hip_kmeans.py::test_seeding_picks_the_oracles_indices: exact
            o = KO.seed(X, c["M"], u)
            idx = np.asarray(o[0] if isinstance(o, tuple) else o)
            np.testing.assert_array_equal(out["idx"].cpu().numpy(), idx)
            np.testing.assert_array_equal(out["C"].cpu().numpy(), X.astype(np.float64)[idx])
        elif nm == "assign":      # test_assignment_paths: labels and d2 bit for bit, inertia rel 1e-12
            import pytest
            want, want_d2 = KO.assign(X, C0)
            np.testing.assert_array_equal(out["labels"].cpu().numpy(), want)
            np.testing.assert_array_equal(out["d2"].cpu().numpy(), want_d2)
            assert float(out["inertia"]) == pytest.approx(float(want_d2.sum()), rel=1e-12)
        else:                     # test_edges_one_iteration_and_assign, three iterations: labels exact, centres atol 1e-12
            Cc, labels = C0, None
            for _ in range(3):
                Cc, labels, _, _ = KO.lloyd_iter(X, Cc)
            np.testing.assert_array_equal(out["labels"].cpu().numpy(), labels)
            np.testing.assert_allclose(out["C"].cpu().numpy(), Cc, rtol=0, atol=1e-12 * max(1.0, np.abs(Cc).max()))
            assert int(out["state"][0]) == 3
    return check


def _kmeans_bytes(nm, w):
    N, M = KMEANS_SHAPES[w]
    extra = (KO.n_trials(M),) if nm == "seed" else ()
    return getattr(_lib().load(), f"gpz_kmeans_{nm}_workspace_bytes")(N, 2, M, *extra)


for _nm, _fn, _ix in (("seed", _kmeans_seed_run, dict(idx=lambda c: c["N"])),
                      ("lloyd", _kmeans_lloyd_run, dict(labels=lambda c: c["M"])),
                      ("assign", _kmeans_assign_run, dict(labels=lambda c: c["M"]))):
    add(Row(f"kmeans_{_nm}", (f"gpz_kmeans_{_nm}",), KMEANS_SHAPES, _kmeans_build, _fn, F32, index=_ix, slices=_kmeans_slices,
            check=_kmeans_check(_nm),
            bytes=functools.partial(_kmeans_bytes, _nm)))


# =====================================================================================================================
# Gram entry: gpz_kernel_gram (csrc/gram.hip).  ops.kernel_gram_plan: SMALL (N, M) = (70, 20) in fp32 is one tile and one
# N-split; LARGE (3000, 300) is three row blocks and 24 splits of 128 columns, the last of 56.  A scalar-parameter kernel
# gives one Gram matrix and R = 3 right-hand sides; the per-latent kernel gives n = 3 matrices with R = 1.
# =====================================================================================================================

GRAM_SHAPES = dict(small=(70, 20), large=(3000, 300))


def _gram_build(which):
    N, M = GRAM_SHAPES[which]
    g = _gen(N, M, 3)
    return dict(Z=_rand(g, M, 2) * 8 - 4, X=_rand(g, N, 2) * 8 - 4, F=_randn(g, 3, N), sigma=torch.tensor([1.25, 0.75, 1.5]),
                ell=torch.tensor([1.5, 2.0, 1.0]))


def _gram_run(ops, s, batched):
    sig, ell = (s["sigma"], s["ell"]) if batched else (s["sigma"][:1], s["ell"][:1])
    G, b = ops.kernel_gram(ops.KernelSpec(EC.KIND_ID["rbf"], sig, ell, batched), s["Z"], s["X"], s["F"], 1e-5)
    return dict(G=G, b=b)


def _gram_check(batched):
    def check(which, c, out):
        # tests/test_hip_projection.py::test_gram_and_rhs_match_the_oracle, fp32: tol 1e-4 of |ref| + 1e-4 of max diag(G)
        # (of max|b| for b), G exactly symmetric
        # (the oracle's kernel matrix and the two products of projection_oracle.project; its solve is not needed here)
        import projection_oracle as PO
        sig, ell = (c["sigma"], c["ell"]) if batched else (c["sigma"][0], c["ell"][0])
        Kzx = PO.kernel_matrix("rbf", c["Z"], c["X"], sig, ell)
        K3, F = (Kzx if batched else Kzx[None]), c["F"].double()
        o = dict(G=K3 @ K3.transpose(-1, -2) + 1e-5 * torch.eye(K3.shape[-2], dtype=F64),
                 b=(K3 @ F[:, :, None]).transpose(-1, -2) if batched else (F @ Kzx.t())[None])
        G, b = out["G"].cpu(), out["b"].cpu()
        assert torch.equal(G, G.transpose(-1, -2))
        for got, want, scale in ((G, o["G"].reshape(G.shape), float(torch.diagonal(o["G"], dim1=-2, dim2=-1).max())),
                                 (b, o["b"].reshape(b.shape), float(o["b"].abs().max()))):
            assert bool(((got - want).abs() <= 1e-4 * want.abs() + 1e-4 * scale).all())
    return check


def _gram_slices(w):
    from gpzoo_amd import ops
    N, M = GRAM_SHAPES[w]
    return dict(n_splits=ops.kernel_gram_plan(N, M, 1, F32)["n_splits"], row_blocks=cdiv(M, 128))


for _b in (False, True):
    add(Row("kernel_gram-{}".format("per_latent" if _b else "R3"), ("gpz_kernel_gram",), GRAM_SHAPES, _gram_build,
            functools.partial(_gram_run, batched=_b), F32, slices=_gram_slices, check=_gram_check(_b),
            bytes=lambda w, b=_b: _lib().load().gpz_kernel_gram_workspace_bytes(*GRAM_SHAPES[w], 3 if b else 1, 1 if b else 3,
                                                                                _code(F32))))


# =====================================================================================================================
# dense KL NMF: gpz_nmf_kl_update, gpz_nmf_kl_divergence (csrc/nmf.hip).  nmf_plan: wblocks = ceil(N / 64), cblocks =
# ceil(D / 256), slabs of whole 64-row chunks, min(ceil(1024 / cblocks), wblocks) of them.  LARGE (N, D, L) =
# (300, 300, 5): five W blocks = five slabs (the last of 44 rows), two column blocks (the last of 44 columns).
# =====================================================================================================================

NMF_SHAPES = dict(small=(50, 37, 5), large=(300, 300, 5))


def _nmf_build(dtype, which):
    N, D, L = NMF_SHAPES[which]
    rng = np.random.default_rng([N, D, L])
    X = NO.planted_counts(N, D, L, 11 + N)
    W0, H0 = np.abs(rng.standard_normal((N, L))) + 0.05, np.abs(rng.standard_normal((L, D))) + 0.05
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)      # noqa: E731
    return dict(X=f(X), W0=f(W0), H0=f(H0))


def _nmf_run(ops, s):
    W, H, n = ops.nmf_kl_mu(s["X"], s["W0"], s["H0"], max_iter=3, tol=0.0)
    return dict(W=W, H=H, divergence=torch.tensor(ops.nmf_kl_divergence(s["X"], W, H), dtype=F64))


def _nmf_iterates_check(dtype, X, W0, H0, out, what):
    """Three oracle updates from the same start.  fp64: tests/test_hip_nmf.py::close(rtol 1e-5, atol 1e-5 max|ref|); fp32:
    that file's rule for fp32, four times the distance of the reference's own fp32 evaluation from its fp64 one (here
    nmf_oracle run in float32), for W, H and W H; the divergence of the result: rel 1e-10 / 1e-5 (test_divergence)."""
    def iterate(t):
        W, H = W0.astype(t), H0.astype(t)
        for _ in range(3):
            W = NO.update_w(X.astype(t), W, H)
            H = NO.update_h(X.astype(t), W, H)
        return W.astype(np.float64), H.astype(np.float64)
    W, H = iterate(np.float64)
    Wg, Hg = out["W"].double().cpu().numpy(), out["H"].double().cpu().numpy()
    assert np.isfinite(Wg).all() and np.isfinite(Hg).all()
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())      # noqa: E731
    if dtype == F64:
        for nm, g, r in (("W", Wg, W), ("H", Hg, H)):
            assert (np.abs(g - r) <= 1e-5 * np.abs(r) + 1e-5 * np.abs(r).max()).all(), (what, nm)
    else:
        W32, H32 = iterate(np.float32)
        for nm, got, delta in (("W", rel(Wg, W), rel(W32, W)), ("H", rel(Hg, H), rel(H32, H)),
                               ("WH", rel(Wg @ Hg, W @ H), rel(W32 @ H32, W @ H))):
            print(what, nm, f"kernel {got:.3e}, the oracle's own fp32 noise {delta:.3e}")
            assert got <= 4 * delta, (what, nm, got, delta)
    want = NO.kl_divergence(X, Wg, Hg)
    assert abs(float(out["divergence"]) - want) <= (1e-10 if dtype == F64 else 1e-5) * want


def _nmf_check(dtype):
    def check(which, c, out):
        _nmf_iterates_check(dtype, *(c[k].double().numpy() for k in ("X", "W0", "H0")), out, f"nmf_kl {which}")
    return check


def _nmf_slices(w):
    N, D, _ = NMF_SHAPES[w]
    wb, cb = cdiv(N, 64), cdiv(D, 256)
    want = max(1, min(cdiv(1024, cb), wb))
    slab_rows = cdiv(cdiv(N, want), 64) * 64
    return dict(w_blocks=wb, column_blocks=cb, slabs=cdiv(N, slab_rows))


for _dt, _nm in ((F32, "f32"), (F64, "f64")):
    add(Row(f"nmf_kl-{_nm}", ("gpz_nmf_kl_update", "gpz_nmf_kl_divergence"), NMF_SHAPES, functools.partial(_nmf_build, _dt),
            _nmf_run, _dt, slices=_nmf_slices, check=_nmf_check(_dt),
            bytes=lambda w, dt=_dt: _lib().load().gpz_nmf_kl_workspace_bytes(*NMF_SHAPES[w], _code(dt))))


# =====================================================================================================================
# sparse counts: the case builder of sparse_poisson_cases.  The gene passes split a gene's row into chunks of
# ``gene_chunk`` (512) non-zeros: SMALL has 70 spots, so every row is one chunk; LARGE gives gene 3 a full row of 1030
# non-zeros -- three chunks, the last of 6 -- and gene 5 a row of 513, two chunks with a one-entry tail.
# =====================================================================================================================

SP_SMALL, SP_LARGE = (70, 37, 20, 2), (1030, 515, 20, 2)             # (N, D, Lt, E); LARGE is nb_cases' LARGE below
SP_SHAPES = dict(small=SP_SMALL, large=SP_LARGE)
SP_BATCH = dict(small=33, large=517)                                  # spots of the batch rows (an unsorted idx)


def _sparse_rows(which):
    N = SP_SHAPES[which][0]
    return {3: list(range(N)), 5: list(range(0, N, 2))[:513]} if which == "large" else {}


@functools.lru_cache(maxsize=None)
def _sparse_build(which, E=None, batch=False, theta=False):
    N, D, Lt, E0 = SP_SHAPES[which]
    E = E or E0
    idx = None
    if batch:
        idx = torch.randperm(N, generator=_gen(N, 3))[:SP_BATCH[which]].tolist()
    kw = dict(density=0.05, idx=idx, rows=_sparse_rows(which))
    c = SNC.make_nb_case(N, D, Lt, E, 21, **kw) if theta else SPC.make_sparse_case(N, D, Lt, E, 21, **kw)
    c.setdefault("stored_zeros", [])
    return c


def _sparse_prepare(c):
    from gpzoo_amd.likelihoods import SparseCounts
    s = {k: (v.float().cuda() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in c.items()}
    s["counts"] = SparseCounts(c["y"].float()).cuda()
    s["idx_dev"] = c["idx"].cuda() if "idx" in c else None
    return s


def _sparse_slices(plan_of):
    def slices(w):
        c_rows = _sparse_rows(w)
        longest = max([len(v) for v in c_rows.values()] + [1])
        N, D, Lt, E = SP_SHAPES[w]
        p = plan_of(N, D, Lt, E)
        out = dict(chunks_of_longest_gene=cdiv(longest, p["gene_chunk"]))
        for k in ("gene_slices", "spot_slices"):
            if k in p:
                out[k] = p[k]
        return out
    return slices


def _psp_run(ops, s, with_lgamma):
    o = ops.poisson_nsf_sparse(s["mean"], s["scale"], s["eps"], s["W"], s["V"], s["counts"], idx=s["idx_dev"],
                               with_lgamma=with_lgamma)
    return dict(zip(("ll",) + PC.OUTPUTS, o))


def _psp_check(with_lgamma):
    def check(which, c, out):                       # tests/test_hip_poisson_sparse.py: poisson_cases' tolerances
        ref = SPC.reference(c, with_lgamma)
        for k in ("ll",) + PC.OUTPUTS:
            _close(out[k].reshape(ref[k].shape if k != "ll" else ()), torch.as_tensor(ref[k]), PC.tolerance(ref, k),
                   f"poisson_nsf_sparse {which} {k}")
    return check


def _sparse_nnz(which) -> int:
    return int((_sparse_build(which)["y"] > 0).sum())      # the counts do not depend on E, the batch or theta


def _sp_plan(name, batch=False, E=None):
    def plan_of(N, D, Lt, E0):
        from gpzoo_amd import ops
        which = "small" if N == SP_SMALL[0] else "large"
        return getattr(ops, name)(N, SP_BATCH[which] if batch else N, D, Lt, E or E0, _sparse_nnz(which))
    return plan_of


for _batch, _lg in ((False, True), (True, False)):
    add(Row("poisson_nsf_sparse-{}-{}".format("batch" if _batch else "full", "lgamma" if _lg else "no_lgamma"),
            ("gpz_poisson_nsf_sparse",), SP_SHAPES, functools.partial(_sparse_build, batch=_batch),
            functools.partial(_psp_run, with_lgamma=_lg), F32, prepare=_sparse_prepare, check=_psp_check(_lg),
            slices=_sparse_slices(_sp_plan("poisson_nsf_sparse_plan", _batch)),
            bytes=lambda w, b=_batch: _sp_plan("poisson_nsf_sparse_plan", b)(*SP_SHAPES[w])["workspace_bytes"]))


NB_GRADS = ("mean", "scale", "W", "V", "theta")


def _nbsp_run(ops, s, with_lgamma):
    o = ops.nb_nsf_sparse(s["mean"], s["scale"], s["eps"], s["W"], s["V"], s["theta"], s["counts"], idx=s["idx_dev"],
                          with_lgamma=with_lgamma)
    return dict(zip(("ll",) + tuple("d" + k for k in NB_GRADS), o))


def _nbsp_check(with_lgamma):
    def check(which, c, out):                       # tests/test_hip_nb_sparse.py::check -> nb_cases.check
        ref, grads = SNC.reference(c, with_lgamma)
        NBC.check(out["ll"], {k: out["d" + k] for k in NB_GRADS}, ref, grads, f"nb_nsf_sparse {which}")
    return check


for _batch, _lg, _E in ((False, True, None), (True, False, None), (False, True, 33)):
    add(Row("nb_nsf_sparse-{}-{}{}".format("batch" if _batch else "full", "lgamma" if _lg else "no_lgamma",
                                           "-E33" if _E else ""),
            ("gpz_nb_nsf_sparse",), SP_SHAPES, functools.partial(_sparse_build, batch=_batch, theta=True, E=_E),
            functools.partial(_nbsp_run, with_lgamma=_lg), F32, prepare=_sparse_prepare, check=_nbsp_check(_lg),
            slices=_sparse_slices(_sp_plan("nb_nsf_sparse_plan", _batch, _E)),
            bytes=lambda w, b=_batch, e=_E: _sp_plan("nb_nsf_sparse_plan", b, e)(*SP_SHAPES[w])["workspace_bytes"]))


# =====================================================================================================================
# dense Poisson and NB steps: gpz_poisson_nsf (poisson_cases.SMALL / LARGE, the shapes of
# test_hip_poisson_forms.py::test_bitwise_reproducible_across_workspace_reuse, which stays), gpz_nb_nsf at
# D = 515, N = 1030, Lt = 20, E = 2: nb_plan gives S = 2 gene slices (ceil(D / 512) = 2, 1536 / (17 * 2) is larger) and
# SN = 3 spot slices (ceil(N / 512)); N mod 4 = 2 is the unaligned path and KS = 5 the tail instance.  E = 33 makes the host
# split into a call of 32 samples and a call of one.
# =====================================================================================================================

POISSON_SHAPES = dict(small=PC.SMALL, large=PC.LARGE)


def _poisson_build(which):
    return PC.make_case(*PC.SMALL) if which == "small" else PC.make_probe_case(*PC.LARGE)


def _dense_prepare(c):
    return {k: (v.float().cuda() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in c.items()}


def _poisson_run(ops, s):
    return dict(zip(("ll",) + PC.OUTPUTS, ops.poisson_nsf(s["mean"], s["scale"], s["eps"], s["W"], s["V"], s["y"], True)))


def _poisson_check(which, c, out):                  # tests/test_hip_poisson_forms.py::check
    ref = PC.reference(c, True)
    for k in ("ll",) + PC.OUTPUTS:
        _close(out[k], torch.as_tensor(ref[k]), PC.tolerance(ref, k), f"poisson_nsf {which} {k}")


POISSON_SLICED = dict(small=PC.SMALL, large=(1030, 515, 20, 2))       # the NB step's LARGE: S = 2 gene slices, SN = 3 spot slices


def _poisson_slices(shapes):
    def slices(w):
        p = PC.plan(*shapes[w])
        out = dict(spot_slices=p["SN"])
        if shapes is POISSON_SLICED:      # poisson_cases.LARGE has 20 genes: one gene slice, 16 spot slices (the last empty)
            out["gene_slices"] = p["S"]
        return out
    return slices


def _poisson_build_of(shapes, which):
    if shapes is POISSON_SHAPES:
        return _poisson_build(which)
    return PC.make_case(*shapes[which], seed=3)


for _nm, _sh in (("poisson_nsf", POISSON_SHAPES), ("poisson_nsf-gene_slices", POISSON_SLICED)):
    add(Row(_nm, ("gpz_poisson_nsf",), _sh, functools.partial(_poisson_build_of, _sh), _poisson_run, F32, prepare=_dense_prepare,
            check=_poisson_check, slices=_poisson_slices(_sh), bytes=lambda w, sh=_sh: PC.workspace_bytes(*sh[w])))

NB_SHAPES = dict(small=(70, 37, 20, 2), large=(1030, 515, 20, 2))     # (N, D, Lt, E)


def _nb_build(which, E=None):
    N, D, Lt, E0 = NB_SHAPES[which]
    return NBC.make_inputs(D, N, Lt, E or E0, seed=5)


def _nb_run(ops, s, with_lgamma):
    o = ops.nb_nsf(s["mean"], s["scale"], s["eps"], s["W"], s["V"], s["theta"], s["y"], with_lgamma)
    return dict(zip(("ll",) + tuple("d" + k for k in NB_GRADS), o))


def _nb_check(with_lgamma):
    def check(which, c, out):                       # tests/test_hip_nb.py -> nb_cases.check
        ref, grads = NBC.oracle(c, with_lgamma)
        NBC.check(out["ll"], {k: out["d" + k] for k in NB_GRADS}, ref, grads, f"nb_nsf {which}")
    return check


def _nb_slices(w):
    from gpzoo_amd import ops
    p = ops.nb_nsf_plan(*NB_SHAPES[w])
    return dict(gene_slices=p["gene_slices"], spot_slices=p["spot_slices"])


for _lg, _E in ((True, None), (False, None), (True, 33)):
    add(Row("nb_nsf-{}{}".format("lgamma" if _lg else "no_lgamma", "-E33" if _E else ""), ("gpz_nb_nsf",), NB_SHAPES,
            functools.partial(_nb_build, E=_E), functools.partial(_nb_run, with_lgamma=_lg), F32, prepare=_dense_prepare,
            check=_nb_check(_lg), slices=_nb_slices,
            bytes=lambda w: _lib().load().gpz_nb_nsf_workspace_bytes(*NB_SHAPES[w])))


# =====================================================================================================================
# deviance entries: gpz_poisson_deviance, gpz_nb_deviance and their sparse forms (csrc/deviance.hip, nb_deviance.hip).
# The plans (ops.poisson_deviance_plan, ops.nb_deviance_plan) report gene_slices = ceil(D / 64) and spot_slices; LARGE
# (N, D, Lt) = (1100, 150, 5) is three gene slices (the last of 22 genes) and three spot slices of six tiles (the last of
# six, with a 12-spot last tile); N = 1100 > 512 gives the sparse forms a gene row of more than one chunk.
# =====================================================================================================================

DEV_SHAPES = dict(small=(70, 37, 5), large=(1100, 150, 5))            # (N, D, Lt)


def _dev_build(which, nb=False):
    return (NDC if nb else DC).make_case(*DEV_SHAPES[which], seed=2)


def _dev_prepare(c):
    from gpzoo_amd.likelihoods import SparseCounts
    s = _dense_prepare(c)
    s["counts"] = SparseCounts(c["y"].float()).cuda()
    return s


def _dev_run(ops, s, nb, sparse):
    a = [s["mean"], s["scale"], s["W"], s["V"]] + ([s["theta"]] if nb else [])
    fn = getattr(ops, ("nb" if nb else "poisson") + "_deviance" + ("_sparse" if sparse else ""))
    return dict(fn(*a, s["counts"] if sparse else s["y"]))


def _dev_check(nb):
    def check(which, c, out):                       # tests/test_hip_deviance.py, tests/test_hip_nb_deviance.py::check
        M = NDC if nb else DC
        fig = M.figures(M.oracle(c, True), out)
        print("deviance", which, {k: f"{v:.3g}" for k, v in fig.items()})
        for k, v in fig.items():
            assert v <= 1.0, (which, k, v)
    return check


def _dev_slices(nb, sparse):
    def slices(w):
        from gpzoo_amd import ops
        N, D, Lt = DEV_SHAPES[w]
        if sparse:
            p = getattr(ops, ("nb" if nb else "poisson") + "_deviance_sparse_plan")(N, N, D, Lt, N * D)
            return dict(chunks_of_longest_gene=cdiv(int((_inputs_dev(w, nb)["y"] > 0).sum(1).max()), p["gene_chunk"]))
        p = getattr(ops, ("nb" if nb else "poisson") + "_deviance_plan")(N, D, Lt)
        return dict(gene_slices=p["gene_slices"], spot_slices=p["spot_slices"])
    return slices


@functools.lru_cache(maxsize=None)
def _inputs_dev(which, nb):
    return _dev_build(which, nb)


def _dev_bytes(nb, sparse):
    def nbytes(w):
        from gpzoo_amd import ops
        N, D, Lt = DEV_SHAPES[w]
        name = ("nb" if nb else "poisson") + "_deviance" + ("_sparse" if sparse else "") + "_plan"
        nnz = int((_inputs_dev(w, nb)["y"] > 0).sum())
        return getattr(ops, name)(*((N, N, D, Lt, nnz) if sparse else (N, D, Lt)))["workspace_bytes"]
    return nbytes


for _nb, _sp in itertools.product((False, True), (False, True)):
    _e = "gpz_" + ("nb" if _nb else "poisson") + "_deviance" + ("_sparse" if _sp else "")
    add(Row(_e[4:], (_e,), DEV_SHAPES, functools.partial(_inputs_dev, nb=_nb),
            functools.partial(_dev_run, nb=_nb, sparse=_sp), F32, prepare=_dev_prepare, check=_dev_check(_nb),
            slices=_dev_slices(_nb, _sp), bytes=_dev_bytes(_nb, _sp)))


# =====================================================================================================================
# sparse KL NMF and the count products: gpz_nmf_kl_sparse_update, gpz_nmf_kl_sparse_divergence, gpz_counts_matmul
# (csrc/nmf_sparse.hip).  The counts of the sparse rows above (D genes x N spots; X = counts^T): the gene pass chunks a
# gene's row as there; colsum_rows = 256 rows per block of the partial sums, LARGE has five blocks of spots (the last of 6
# rows) and three of genes (the last of 3).
# =====================================================================================================================

def _snmf_build(dtype, which):
    c = _sparse_build(which)
    N, D, _, _ = SP_SHAPES[which]
    rng = np.random.default_rng([N, D, 9])
    f = lambda a: torch.from_numpy(a).to(dtype)      # noqa: E731
    g = _gen(N, D, 8)
    return dict(y=c["y"], W0=f(np.abs(rng.standard_normal((N, 5))) + 0.05), H0=f(np.abs(rng.standard_normal((5, D))) + 0.05),
                Qd=_randn(g, D, 7, dtype=F64), Qn=_randn(g, N, 7, dtype=F64))


def _snmf_prepare(c):
    from gpzoo_amd.likelihoods import SparseCounts
    s = _to_cuda(c)
    s["counts"] = SparseCounts(c["y"].float()).cuda()
    return s


def _snmf_run(ops, s):
    W, H, n = ops.nmf_kl_mu_sparse(s["counts"], s["W0"], s["H0"], max_iter=3, tol=0.0)
    return dict(W=W, H=H, divergence=torch.tensor(ops.nmf_kl_divergence_sparse(s["counts"], W, H), dtype=F64))


def _snmf_check(dtype):
    def check(which, c, out):                       # the dense entry's check: the oracle's own iterates on the dense X
        _nmf_iterates_check(dtype, c["y"].numpy().T.astype(np.float64), c["W0"].double().numpy(), c["H0"].double().numpy(), out,
                            f"nmf_kl_sparse {which}")
    return check


def _snmf_slices(w):
    N, D, _, _ = SP_SHAPES[w]
    out = _sparse_slices(lambda N, D, Lt, E: _nmf_sparse_plan(N, D))(w)
    cr = _nmf_sparse_plan(N, D)["colsum_rows"]
    out.update(spot_blocks=cdiv(N, cr), gene_blocks=cdiv(D, cr))
    return out


def _nmf_sparse_plan(N, D, dtype=F32):
    from gpzoo_amd import ops
    return ops.nmf_kl_sparse_plan(N, D, 5, _sparse_nnz("small" if N == SP_SMALL[0] else "large"), dtype)


for _dt, _nm in ((F32, "f32"), (F64, "f64")):
    add(Row(f"nmf_kl_sparse-{_nm}", ("gpz_nmf_kl_sparse_update", "gpz_nmf_kl_sparse_divergence"), SP_SHAPES,
            functools.partial(_snmf_build, _dt), _snmf_run, _dt, prepare=_snmf_prepare, slices=_snmf_slices,
            check=_snmf_check(_dt),
            bytes=lambda w, dt=_dt: _nmf_sparse_plan(*SP_SHAPES[w][:2], dtype=dt)["workspace_bytes"]))


def _cm_run(ops, s, transpose):
    return dict(out=ops.counts_matmul(s["counts"], s["Qn"] if transpose else s["Qd"], transpose=transpose))


def _cm_check(transpose):
    def check(which, c, out):                       # tests/test_hip_nmf_sparse.py::test_counts_matmul_both_orientations
        X = c["y"].double().T
        ref = X.T @ c["Qn"] if transpose else X @ c["Qd"]
        assert float((out["out"].cpu() - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    return check


for _t in (False, True):
    add(Row("counts_matmul-{}".format("transpose" if _t else "plain"), ("gpz_counts_matmul",), SP_SHAPES,
            functools.partial(_snmf_build, F32), functools.partial(_cm_run, transpose=_t), F64, prepare=_snmf_prepare,
            check=_cm_check(_t), slices=_sparse_slices(lambda N, D, Lt, E: _nmf_sparse_plan(N, D)) if _t else None,
            bytes=(lambda w: _lib().load().gpz_counts_matmul_workspace_bytes(*SP_SHAPES[w][:2], _sparse_nnz(w), 7, 1))
            if _t else None))          # without the transpose nothing is carved but placeholders


# ---------------------------------------------------------------------------------------------------------------------
# the header
# ---------------------------------------------------------------------------------------------------------------------

# entries that take a workspace but serve diagnostics only (none is declared in include/gpzoo_hip.h today)
DEBUG_PREFIX = "gpz_debug_"


def header_entries_with_workspace(header_text: str) -> set:
    """Every ``gpz_*`` function declared in the header that takes a ``ws`` argument or has a ``_workspace_bytes`` companion."""
    import re
    decls = re.findall(r"\b(gpz_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header_text, flags=re.S)
    names = {n for n, _ in decls}
    out = set()
    for n, args in decls:
        if n.endswith("_workspace_bytes") or n.endswith("_plan") or n.startswith(DEBUG_PREFIX):
            continue
        if re.search(r"\bvoid\s*\*\s*ws\b", args) or (n + "_workspace_bytes") in names:
            out.add(n)
    return out
