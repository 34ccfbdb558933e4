"""GPU: WSVGP.forward_precomputed and gpz_wsvgp_precomputed(_backward) beyond one 128-row block and one chunk -- Mp = 128,
256 and 384, M and N next to the 32 x 32 transpose tile and the 128 pad, the chunk loop of both passes (through the
gpz_debug_precomputed_chunk seam: the 2 GiB rule never cuts at test size), one q(U) shared by the rows of W, the None
upstreams, frozen parameters and a workspace full of NaN -- against the reference's expression (gp.py:308-322) in torch fp64
and its autograd.  Cases and their reasons: tests/entry_cases.py / tests/test_entry_cases.py.

Tolerances: helpers.rtol_for; `scale` with atol = 0 (it is positive), `mean` and the gradients with atol = rtol max|ref|."""
import contextlib
import ctypes as C

import pytest
import torch
import torch.nn as nn

import entry_cases as E
from helpers import rtol_for

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def _seam():
    from gpzoo_amd import _lib
    fn = _lib.load().gpz_debug_precomputed_chunk
    fn.restype, fn.argtypes = C.c_int64, [C.c_int64]
    return fn


@contextlib.contextmanager
def chunk_width(cols):
    """Columns per chunk of the precomputed passes for the duration of the block (0: the library's rule)."""
    fn = _seam()
    prev = fn(cols)
    try:
        assert fn(cols) == cols
        yield
    finally:
        fn(prev)


def _close(got, ref, dtype, what, positive=False):
    rt = rtol_for(dtype)
    ref = ref.reshape(got.shape)
    torch.testing.assert_close(got.double().cpu(), ref, rtol=rt, atol=0.0 if positive else rt * float(ref.abs().max()),
                               msg=lambda m: f"{what}: {m}")


def _gp(c, dtype, sigma_shape="vec"):
    """A WSVGP whose q(U) and kernel sigma are the case's (sigma as a length-L vector, (L,1,1) or a scalar)."""
    import gpzoo.gp as G
    import gpzoo.kernels as K
    sig = c["sigma"]
    if sig.dim() == 0:
        k = K.RBF()
    elif sigma_shape == "nsf":
        k, sig = K.NSF_RBF(L=c["L"]), sig.reshape(-1, 1, 1)
    else:
        k = K.batched_RBF()
    k.sigma = nn.Parameter(sig.clone())
    gp = G.WSVGP(k, dim=2, M=c["M"], jitter=1e-4)
    gp.mu, gp.Lu = nn.Parameter(c["mu"].clone()), nn.Parameter(c["Lu_raw"].clone())
    return gp.to(dtype).cuda()


def _run_module(c, dtype, use_mean=True, use_scale=True, sigma_shape="vec"):
    gp = _gp(c, dtype, sigma_shape)
    qF, qU, pU = gp.forward_precomputed(c["W"].to(dtype).cuda())
    assert pU is None and qF.mean.requires_grad
    loss = 0.0
    if use_mean:
        loss = loss + (qF.mean.reshape(c["L"], c["N"]) * c["R1"].to(dtype).cuda()).sum()
    if use_scale:
        loss = loss + (qF.scale.reshape(c["L"], c["N"]) * c["R2"].to(dtype).cuda()).sum()
    loss.backward()
    return dict(mean=qF.mean.detach(), scale=qF.scale.detach(), Lu=qU.scale_tril.detach(), grad_mu=gp.mu.grad,
                grad_Lu=gp.Lu.grad, grad_sigma=gp.kernel.sigma.grad), gp


def _run_ops(c, dtype):
    from gpzoo_amd import ops
    W, sig, mu, Lur = (c[n].to(dtype).cuda() for n in ("W", "sigma", "mu", "Lu_raw"))
    out = ops.wsvgp_precomputed(W, sig, mu, Lur)
    gmu, gLu, gsig = ops.wsvgp_precomputed_backward(W, sig, mu, Lur, c["R1"].to(dtype).cuda(), c["R2"].to(dtype).cuda(), out["scale"])
    assert gsig.dtype == F64
    return dict(mean=out["mean"], scale=out["scale"], Lu=out["Lu"], grad_mu=gmu, grad_Lu=gLu, grad_sigma=gsig)


def _check(got, ref, dtype, what, names=("mean", "scale", "Lu", "grad_mu", "grad_Lu", "grad_sigma")):
    for n in names:
        assert got[n] is not None and torch.isfinite(got[n]).all(), f"{what}: {n}"
        _close(got[n], ref[n], dtype, f"{what}: {n}", positive=n == "scale")


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("clamped", [True, False])
@pytest.mark.parametrize("shape", E.PRE_SHAPES)
def test_precomputed_moments_and_gradients(shape, clamped, dtype):
    """Through gp.forward_precomputed and through ops.wsvgp_precomputed(_backward).  (L, N, M): (1,1,1) everything padding but
    one element; (2,129,33) / (2,128,32) one past and exactly on the transpose tile and the pad; (3,257,129) and (2,1300,130)
    Mp = 256 (two row tiles of the upper-triangular LuT product, three lower tiles of G); (2,300,257) Mp = 384.
    fp32 accumulates G with wide_nt_launch; the precomputed pass hands it no scratch, so its k extent (the chunk's columns)
    is never cut into pieces here -- and wide_nt_pieces itself says 1 for every shape of this list (Mp <= 384 gives at most 6
    tiles per latent, and a piece needs 1024 columns: the widest chunk here is pad(1300) = 1408 < 2048).  The cut pieces run
    under the fused backward's tests, which pass the scratch (tests/test_hip_backward_forms.py)."""
    c = E.precomputed_case(*shape, clamped=clamped)
    ref = E.precomputed_ref(c)
    assert bool((ref["prior"] < 0).any()) == (clamped and shape[1] >= 4)
    _check(_run_ops(c, dtype), ref, dtype, f"ops {shape}")
    for sigma_shape in ("vec", "nsf"):
        got, _ = _run_module(c, dtype, sigma_shape=sigma_shape)
        _check(got, ref, dtype, f"module {shape} sigma {sigma_shape}")


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("M", E.CHUNK_M)
@pytest.mark.parametrize("N", E.CHUNK_N)
def test_chunk_loop_of_both_passes(N, M, dtype):
    """Chunk widths 128 and 256 on N = 256 (two exact chunks / one), 300 (a ragged third / second) and 257 (a last chunk of
    one column): n0 > 0, G accumulating across chunks, mu_part[chunk], sig_direct accumulating, fb0.  Every chunking meets
    the fp64 reference.  Across chunkings (128, 256, the rule's single chunk) `mean` is bitwise equal -- w_rowstats works per
    column -- and is asserted so; on MI355X `scale` and Lu came out bitwise equal too, in every one of these cases and both
    precisions (the column sums of squares are per column as well).  The gradients differ by rounding only."""
    from gpzoo_amd import _lib, ops
    lib = _lib.load()
    cases = {w: c for n, m, w, c in E.chunk_cases() if (n, m) == (N, M)}
    c = cases[E.CHUNK_WIDTHS[0]]
    ref = E.precomputed_ref(c)
    runs, nbytes = {}, {}
    for w in E.CHUNK_WIDTHS + (0,):
        with chunk_width(w):
            # the library's own plan, seen through its workspace sizes (ll_part and mu_part grow with the chunk count,
            # Wc / Pc shrink with the chunk width)
            nbytes[w] = (lib.gpz_wsvgp_precomputed_workspace_bytes(c["L"], N, M, ops._dt(c["W"].to(dtype))),
                         lib.gpz_wsvgp_precomputed_backward_workspace_bytes(c["L"], N, M, ops._dt(c["W"].to(dtype))))
            runs[w] = _run_ops(c, dtype)
            _check(runs[w], ref, dtype, f"N={N} M={M} width {w}")
            got, _ = _run_module(c, dtype)
            _check(got, ref, dtype, f"module N={N} M={M} width {w}")
    esz = 4 if dtype == F32 else 8
    rule = E.pre_plan(c["L"], N, M, esz)
    assert rule["nchunks"] == 1
    for w in E.CHUNK_WIDTHS:
        plan = E.pre_plan(c["L"], N, M, esz, w)
        assert plan["nchunks"] == len(E.chunk_columns(N, w))
        # the override reached pre_plan: another chunk width or count gives other workspace sizes, the same plan the same
        same_plan = (plan["nc"], plan["nchunks"]) == (rule["nc"], rule["nchunks"])
        assert (nbytes[w] == nbytes[0]) == same_plan and (same_plan or (nbytes[w][0] < nbytes[0][0] and nbytes[w][1] < nbytes[0][1]))
        assert torch.equal(runs[w]["mean"], runs[0]["mean"])
        for n in ("grad_mu", "grad_Lu", "grad_sigma"):        # rounding only: each chunking is within tolerance of the other
            _close(runs[w][n], runs[0][n].double().cpu(), dtype, f"width {w} vs one chunk: {n}")
    assert nbytes[128] != nbytes[0]
    # the seam is back at the rule
    assert _seam()(0) == 0


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("L,scalar_sigma", [(3, False), (3, True), (1, False)])
def test_one_qu_shared_by_the_rows_of_w(L, scalar_sigma, dtype):
    """mu (M,), Lu (M,M), W (L,N,M): the reference's expression broadcasts to q(F) of shape (L,N) -- also for L = 1, where
    Normal broadcasts its mean (N,) against the scale (1,N) -- and autograd sums the gradients of mu and Lu (and of a scalar
    sigma) over the rows."""
    c = E.precomputed_case(L, 129, 33, shared=True, scalar_sigma=scalar_sigma)
    ref = E.precomputed_ref(c)
    assert ref["mean"].shape == (L, 129) and ref["grad_mu"].shape == (33,) and ref["grad_Lu"].shape == (33, 33)
    gp = _gp(c, dtype)
    W = c["W"].to(dtype).cuda()
    with torch.no_grad():
        qF0, qU0, _ = gp.forward_precomputed(W)
    qF, qU, _ = gp.forward_precomputed(W)
    for q in (qF0, qF):
        assert q.mean.shape == (L, 129) and q.scale.shape == (L, 129)
        _close(q.mean.detach(), ref["mean"], dtype, "mean")
        _close(q.scale.detach(), ref["scale"], dtype, "scale", positive=True)
    assert qU0.scale_tril.shape == (33, 33) and qU.scale_tril.shape == (33, 33)
    _close(qU0.scale_tril, ref["Lu"], dtype, "Lu")
    ((qF.mean * c["R1"].to(dtype).cuda()).sum() + (qF.scale * c["R2"].to(dtype).cuda()).sum()).backward()
    assert gp.mu.grad.shape == (33,) and gp.Lu.grad.shape == (33, 33) and gp.kernel.sigma.grad.shape == c["sigma"].shape
    _check(dict(grad_mu=gp.mu.grad, grad_Lu=gp.Lu.grad, grad_sigma=gp.kernel.sigma.grad), ref, dtype, "shared q(U)",
           names=("grad_mu", "grad_Lu", "grad_sigma"))


@pytest.mark.parametrize("dtype", [F64, F32])
def test_losses_of_one_moment_and_frozen_parameters(dtype):
    """A loss of `mean` alone and of `scale` alone (the other upstream is None); sigma frozen; mu and Lu frozen."""
    c = E.precomputed_case(2, 129, 33)
    for use_mean, use_scale in ((True, False), (False, True)):
        ref = E.precomputed_ref(c, use_mean=use_mean, use_scale=use_scale)
        got, _ = _run_module(c, dtype, use_mean=use_mean, use_scale=use_scale)
        _check(got, ref, dtype, f"mean {use_mean} scale {use_scale}", names=("grad_mu", "grad_Lu", "grad_sigma"))
        if not use_scale:
            assert bool((got["grad_Lu"] == 0).all()) and bool((got["grad_sigma"] == 0).all())
        else:
            assert bool((got["grad_mu"] == 0).all())
    ref = E.precomputed_ref(c)
    W, R1, R2 = (c[n].to(dtype).cuda() for n in ("W", "R1", "R2"))
    for frozen in (("sigma",), ("mu", "Lu")):
        gp = _gp(c, dtype)
        params = dict(sigma=gp.kernel.sigma, mu=gp.mu, Lu=gp.Lu)
        for n in frozen:
            params[n].requires_grad_(False)
        qF, _, _ = gp.forward_precomputed(W)
        ((qF.mean * R1).sum() + (qF.scale * R2).sum()).backward()
        for n, p in params.items():
            assert (p.grad is None) == (n in frozen), n
            if n not in frozen:
                _close(p.grad, ref["grad_" + n], dtype, f"frozen {frozen}: grad_{n}")


@pytest.mark.parametrize("dtype", [F64, F32])
def test_results_do_not_depend_on_what_the_workspace_held(dtype):
    """Both passes on a workspace full of NaN: equal bits, no NaN (several chunks, so the accumulators are in use)."""
    from gpzoo_amd import ops
    c = E.precomputed_case(2, 300, 130)
    with chunk_width(128):
        first = _run_ops(c, dtype)
        dev = first["mean"].device
        ws = ops._workspace(dev, 1)
        ws.fill_(0xFF)                 # every byte set: NaN read as fp32 and as fp64 (the scratch holds both)
        n8 = ws.numel() // 8 * 8
        assert bool(torch.isnan(ws[:n8].view(torch.float32)).all()) and bool(torch.isnan(ws[:n8].view(torch.float64)).all())
        again = _run_ops(c, dtype)
        assert ops._workspace(dev, 1).data_ptr() == ws.data_ptr()
    for n, v in first.items():
        assert torch.isfinite(again[n]).all() and torch.equal(v, again[n]), n
    _check(again, E.precomputed_ref(c), dtype, "NaN workspace")
