"""GPU: Matern-1/2 and Matern-5/2 on every forward and backward path Matern-3/2 takes.

Values and gradients against the reference's own numbers (tests/golden/extra_matern*.npz, written by
make_matern_golden.py from ``batched_Matern32`` subclasses run through the reference) and against tests/matern_oracle.py
(torch CPU, pinned to those fixtures by tests/test_matern_family.py); the paths among themselves bit for bit, as
tests/test_hip_wide.py does for RBF / Matern-3/2.  Tolerances: helpers.rtol_for (1e-5 fp64, 1e-3 fp32); gradients as
tests/test_hip_kernel_grads.py::_close."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import matern_oracle as MO
from helpers import GOLDEN, load_case, rtol_for
from test_hip_kernel_grads import _close

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)      # tests/golden/inputs.py: the seeded inputs the fixtures' generators share

pytestmark = pytest.mark.gpu

KINDS = ("matern12", "matern52")
SIG, ELL = [1.0, 0.8, 1.3], [2.5, 4.0, 6.0]


def _cls(kind):
    import gpzoo.kernels as K
    return {"matern12": K.batched_Matern12, "matern32": K.batched_Matern32, "matern52": K.batched_Matern52}[kind]


def _kernel(kind, dtype, vector):
    if vector:
        k = _cls(kind)()
        k.sigma, k.lengthscale = nn.Parameter(torch.tensor(SIG, dtype=dtype)), nn.Parameter(torch.tensor(ELL, dtype=dtype))
        return k.cuda()
    return _cls(kind)(sigma=0.9, lengthscale=2.0).to(dtype).cuda()


# ---------------------------------------------------------------- kernel matrices
@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_kernel_matrices_match_reference(kind, tag):
    """ops.kfill and the class forward, scalar and vector parameters, against the reference's matrices; diag=True;
    k(Z, Z) with exactly sigma^2 (+ jitter) on its zero-distance diagonal."""
    from gpzoo_amd import _lib, ops
    from gpzoo_amd.kernels import kernel_spec
    z = np.load(os.path.join(GOLDEN, "extra_matern_kernels_only.npz"), allow_pickle=False)
    dt = torch.float64 if tag == "f64" else torch.float32
    tol = dict(rtol=1e-9, atol=1e-9) if tag == "f64" else dict(rtol=1e-4, atol=1e-4)       # test_vmap_kernels_match_reference's
    X, Z = torch.from_numpy(z[f"{tag}_X"]).cuda(), torch.from_numpy(z[f"{tag}_Z"]).cuda()
    kv, ks = _kernel(kind, dt, True), _kernel(kind, dt, False)
    with torch.no_grad():
        Kv, Ks, Kzz = kv(Z, X), ks(Z, X), ks(Z, Z)
    assert Kv.shape == (3, 77, 96) and Ks.shape == (77, 96) and Kv.dtype == dt
    torch.testing.assert_close(Kv.cpu(), torch.from_numpy(z[f"{tag}_{kind}_vec"]), **tol)
    torch.testing.assert_close(Ks.cpu(), torch.from_numpy(z[f"{tag}_{kind}_scalar"]), **tol)
    torch.testing.assert_close(Kzz.cpu(), torch.from_numpy(z[f"{tag}_{kind}_zz"]), **tol)
    s2 = ks.sigma.detach() ** 2
    assert torch.equal(torch.diagonal(Kzz), s2.expand(77))
    spec = kernel_spec(kv, X)
    assert spec.kind == {"matern12": _lib.KERNEL_MATERN12, "matern52": _lib.KERNEL_MATERN52}[kind]
    assert torch.equal(ops.kfill(spec, Z, X), Kv)
    Kj = ops.kfill(spec, Z, Z, jitter=1e-2)
    s2v = kv.sigma.detach() ** 2
    assert torch.equal(torch.diagonal(Kj, dim1=-2, dim2=-1), (s2v + torch.tensor(1e-2, dtype=dt, device="cuda"))[:, None].expand(3, 77))
    off = ~torch.eye(77, dtype=torch.bool, device="cuda")
    assert torch.equal(Kj[:, off], kv(Z, Z).detach()[:, off])
    # diag=True: sigma^2 broadcast, (N,) for scalar and (L, N) for vector parameters
    assert torch.equal(ks(X, X, diag=True), s2.expand(96)) and ks(X, X, diag=True).shape == (96,)
    assert torch.equal(kv(X, X, diag=True), s2v[:, None].expand(3, 96))
    # an fp32 problem written in fp64 (what the factorisation of an fp32 model reads) is the fp64 formula on the fp32 inputs
    if tag == "f32":
        K64 = ops.kfill(spec, Z, X, out_dtype=torch.float64)
        ref = MO.kernel_matrix(kind, Z.cpu().double(), X.cpu().double(), kv.sigma.detach().cpu().double(),
                               kv.lengthscale.detach().cpu().double())
        torch.testing.assert_close(K64.cpu(), ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("d", [1, 3, 4])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", KINDS)
def test_kernel_matrices_in_other_input_dimensions(kind, dtype, d):
    g = torch.Generator().manual_seed(60 + d)
    X = ((torch.rand(50, d, generator=g, dtype=torch.float64) - 0.5) * 8).to(dtype)
    Z = ((torch.rand(37, d, generator=g, dtype=torch.float64) - 0.5) * 8).to(dtype)
    k = _kernel(kind, dtype, True)
    ref = MO.kernel_matrix(kind, X, Z, k.sigma.detach().cpu(), k.lengthscale.detach().cpu())
    with torch.no_grad():
        K = k(X.cuda(), Z.cuda())
    assert K.shape == (3, 50, 37)
    tol = dict(rtol=1e-9, atol=1e-9) if dtype == torch.float64 else dict(rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(K.cpu(), ref, **tol)


# ---------------------------------------------------------------- modules against the reference's goldens
CASES = [f"extra_{k}_{g}_{t}" for k in KINDS for g in ("wsvgp", "svgp") for t in ("f64", "f32")]


def _model(name, c):
    import math
    import gpzoo.gp as G
    from gpzoo.likelihoods import ExactLikelihood
    k = _cls(c["kind"])()
    k.sigma, k.lengthscale = nn.Parameter(c["sigma"].clone()), nn.Parameter(c["lengthscale"].clone())
    M, d = c["Z"].shape
    gp = (G.WSVGP if c["whitened"] else G.SVGP)(k, dim=d, M=M, jitter=c["jitter"])
    gp.Z, gp.mu, gp.Lu = nn.Parameter(c["Z"].clone()), nn.Parameter(c["mu"].clone()), nn.Parameter(c["Lu_raw"].clone())
    model = ExactLikelihood(gp, noise=math.log(math.expm1(c["noise_sd"])))
    return (model.double() if c["X"].dtype == torch.float64 else model.float()).cuda()


_ORACLE_GRADS = {}


def _oracle_grads(name, c):
    """Computed once per case, shared, never modified."""
    if name not in _ORACLE_GRADS:
        _ORACLE_GRADS[name] = MO.grads(c["kind"], c["whitened"], c["X"], c["y"], c["Z"], c["sigma"], c["lengthscale"],
                                       c["mu"], c["Lu_raw"], c["jitter"], c["noise_sd"])
    return _ORACLE_GRADS[name]


@pytest.mark.parametrize("name", CASES)
def test_module_forward_matches_reference(name):
    """SVGP / WSVGP + ExactLikelihood: mean, scale, kl and elbo of the reference (as test_hip_api.py checks the shipped kinds)."""
    c = load_case(name)
    model = _model(name, c)
    X, y = c["X"].cuda(), c["y"].cuda()
    with torch.no_grad():
        pY, qF, qU, pU = model(X=X, E=1)
        Kzx = model.gp.kernel(model.gp.Z, X)
    rt = rtol_for(X.dtype)
    torch.testing.assert_close(Kzx.cpu(), c["Kzx"], rtol=rt, atol=rt * 1e-1)
    torch.testing.assert_close(qF.mean.cpu(), c["mean"], rtol=rt, atol=rt * 1e-1)
    torch.testing.assert_close(qF.scale.cpu(), c["scale"], rtol=rt, atol=rt * 1e-1)
    torch.testing.assert_close(qU.scale_tril.cpu(), c["Lu"], rtol=rt, atol=rt * 1e-2)
    if c["whitened"]:
        assert pU is None
        from gpzoo.utilities import whitened_KL_batched
        kl = whitened_KL_batched(qU.mean, qU.scale_tril)
    else:
        torch.testing.assert_close(pU.scale_tril.cpu(), c["chol"], rtol=rt, atol=rt * 1e-2)
        kl = torch.distributions.kl_divergence(qU, pU)
    torch.testing.assert_close(kl.cpu().reshape(c["kl"].shape), c["kl"], rtol=rt, atol=rt)
    assert float(model.elbo(X, y)) == pytest.approx(c["elbo"], rel=rt)


def _loss_backward(model, X, y, whitened):
    from gpzoo.utilities import whitened_KL_batched
    model.zero_grad()
    pY, qF, qU, pU = model(X=X, E=1)
    s = torch.nn.functional.softplus(model.noise)
    kl = whitened_KL_batched(qU.mean, qU.scale_tril).sum() if whitened else torch.distributions.kl_divergence(qU, pU).sum()
    loss = -(pY.log_prob(y).sum() - (qF.scale ** 2).sum() / (2 * s ** 2) - kl)
    loss.backward()
    gp = model.gp
    return [gp.mu.grad.clone(), gp.Lu.grad.clone(), gp.kernel.sigma.grad.clone(), gp.kernel.lengthscale.grad.clone(), gp.Z.grad.clone()]


@pytest.mark.parametrize("name", CASES)
def test_module_backward_matches_reference_and_oracle(name):
    """loss.backward() with everything trainable: the reference's autograd gradients for mu, Lu, sigma, lengthscale; Z.grad
    finite (the reference's is NaN) and the oracle's; two runs give identical bits."""
    c = load_case(name)
    model = _model(name, c)
    X, y = c["X"].cuda(), c["y"].cuda()
    dt = X.dtype
    g1 = _loss_backward(model, X, y, c["whitened"])
    g2 = _loss_backward(model, X, y, c["whitened"])
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    for got, key in zip(g1, ("grad_mu", "grad_Lu", "grad_sigma", "grad_lengthscale")):
        _close(got, c[key], dt, key)
    assert torch.isfinite(g1[4]).all()
    _close(g1[4], _oracle_grads(name, c)["grad_Z"], dt, "grad_Z")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", KINDS)
def test_stand_alone_kernel_gradients(kind, dtype):
    """kernel(X, Z).sum().backward() and kernel(X, X).sum().backward() (zero-distance diagonal: finite, the oracle's
    masked-sqrt value), to sigma, lengthscale and the points."""
    from inputs import make_inputs
    inp = make_inputs(311, N=50, M=14, d=2, L=3)
    X0, Z0 = inp["X"].to(dtype), inp["Z"].to(dtype)
    P = torch.cat([X0, Z0]).double()
    assert float((torch.cdist(P, P) + 9 * torch.eye(64, dtype=torch.float64)).min()) >= 2.5e-3   # away from the ill-conditioned unit vector
    for second in ("Z", "X"):
        k = _kernel(kind, dtype, True)
        Xg = X0.cuda().requires_grad_(True)
        Zg = Z0.cuda().requires_grad_(True) if second == "Z" else Xg
        k(Xg, Zg).sum().backward()
        s = torch.tensor(SIG, dtype=dtype, requires_grad=True)
        e = torch.tensor(ELL, dtype=dtype, requires_grad=True)
        Xr = X0.clone().requires_grad_(True)
        Zr = Z0.clone().requires_grad_(True) if second == "Z" else Xr
        MO.kernel_matrix(kind, Xr, Zr, s, e).sum().backward()
        for got, ref, nm in ((Xg.grad, Xr.grad, "X"), (k.sigma.grad, s.grad, "sigma"), (k.lengthscale.grad, e.grad, "lengthscale")):
            assert torch.isfinite(got).all(), nm
            _close(got, ref, dtype, f"{nm} (k(X, {second}))")
        if second == "Z":
            assert torch.isfinite(Zg.grad).all()
            _close(Zg.grad, Zr.grad, dtype, "Z")
    # points that coincide exactly across the two sets: nu = 1/2 returns 0 at the kink, nu = 5/2 its true derivative 0
    k = _kernel(kind, dtype, False)
    A = X0[:5].cuda().requires_grad_(True)
    k(A, X0[:5].cuda()).diagonal().sum().backward()
    assert torch.equal(A.grad, torch.zeros_like(A.grad))


# ---------------------------------------------------------------- the fp32 product paths
def _problem(kind, N, M, L, d, dtype=torch.float32):
    from gpzoo_amd.configs import spec_for_config
    from gpzoo_amd.synthetic import make_config
    c = make_config(3, N=N, M=M, L=L, dtype=dtype, kind=kind)
    if d == 1:
        c["X"], c["Z"] = c["X"][:, :1].contiguous(), c["Z"][:, :1].contiguous()
    g = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    spec, extra = spec_for_config(g, torch.device("cuda", 0))
    return c, g, spec, extra


def _run(c, g, spec, extra, retain=0.9, **kw):
    from gpzoo_amd import ops
    return ops.svgp_forward(spec, g["X"], g["Z"], g["mu"], g["Lu_raw"], c["jitter"], c["whitened"], y=g["y"],
                            noise_sd=c["noise_sd"], want_Lu=False, retain_wt=retain, **extra, **kw)


def _same_numbers(out, ref):
    torch.testing.assert_close(out["mean"], ref["mean"], rtol=1e-5, atol=1e-5 * float(ref["mean"].abs().max()))
    torch.testing.assert_close(out["scale"], ref["scale"], rtol=1e-5, atol=0)
    assert float(out["elbo"]) == pytest.approx(float(ref["elbo"]), rel=1e-7)
    assert torch.equal(out["kl"], ref["kl"])


PATH_SHAPES = [(777, 100, 2, 2),        # a single block
               (2000, 384, 3, 2),       # partial last row tile of both tile heights
               (1500, 640, 2, 1),       # 1-D, five blocks
               (5000, 2048, 1, 2)]      # ragged last column tile


@pytest.mark.parametrize("N,M,L,d", PATH_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_paths_agree_bitwise_in_wt(kind, N, M, L, d):
    """narrow tiles + fill, the default, wide tiles + fill and the generated operand: Wt bit for bit, the moments to fp32
    rounding; and the library's own choice of path is the one it makes for Matern-3/2 at this shape (no fallback)."""
    c, g, spec, extra = _problem(kind, N, M, L, d)
    Mp, ncp = (M + 127) // 128 * 128, (N + 127) // 128 * 128
    nwt = L * Mp * ncp
    ref = _run(c, g, spec, extra, materialize_kzx=True, narrow_tiles=True)
    wref = ref["wt_cache"].view(torch.int32)[:nwt]
    assert int(wref.count_nonzero()) > nwt // 4
    c32, g32, spec32, extra32 = _problem("matern32", N, M, L, d)
    for kw in (dict(), dict(materialize_kzx=True), dict(materialize_kzx=False)):
        out = _run(c, g, spec, extra, **kw)
        assert torch.equal(out["wt_cache"].view(torch.int32)[:nwt], wref), kw
        _same_numbers(out, ref)
        assert out["path"] == _run(c32, g32, spec32, extra32, **kw)["path"], kw
    assert _run(c, g, spec, extra, materialize_kzx=False)["path"] & 2          # the generated operand was taken


PANEL_SHAPES = [(64, 40, 1, 2),         # one panel
                (777, 100, 2, 2),
                (5000, 500, 5, 2),      # Mp = 512 with padded rows and a ragged last panel
                (4000, 333, 3, 1)]


@pytest.mark.parametrize("N,M,L,d", PANEL_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_panel_kernel_agrees_with_the_tile_kernels(kind, N, M, L, d):
    c, g, spec, extra = _problem(kind, N, M, L, d)
    Mp, ncp = (M + 127) // 128 * 128, (N + 127) // 128 * 128
    nwt = L * Mp * ncp
    ref = _run(c, g, spec, extra, materialize_kzx=True)
    out = _run(c, g, spec, extra, panel_products=True)
    assert ref["path"] in (0, 1) and out["path"] == 4
    assert torch.equal(out["wt_cache"].view(torch.int32)[:nwt], ref["wt_cache"].view(torch.int32)[:nwt])
    _same_numbers(out, ref)
    c32, g32, spec32, extra32 = _problem("matern32", N, M, L, d)
    for retain in (0.9, 0.0):           # left to itself: Matern-3/2's path at this shape, retained Wt or not
        assert _run(c, g, spec, extra, retain=retain)["path"] == _run(c32, g32, spec32, extra32, retain=retain)["path"]
    bare = _run(c, g, spec, extra, retain=0.0, panel_products=True)
    assert bare["path"] == 4 and "wt_cache" not in bare
    assert torch.equal(bare["mean"], out["mean"]) and torch.equal(bare["scale"], out["scale"])


@pytest.mark.parametrize("kind", KINDS)
def test_generated_operand_does_not_read_the_kzx_buffer(kind):
    from gpzoo_amd import ops
    c, g, spec, extra = _problem(kind, 6000, 1024, 2, 2)
    a = _run(c, g, spec, extra, materialize_kzx=True)
    assert ops._workspaces
    for t in ops._workspaces.values():
        t.fill_(0xFF)
    b = _run(c, g, spec, extra, materialize_kzx=False)
    assert b["path"] & 2
    nwt = 2 * 1024 * 6016
    assert torch.equal(a["wt_cache"].view(torch.int32)[:nwt], b["wt_cache"].view(torch.int32)[:nwt])
    assert torch.isfinite(b["mean"]).all() and torch.isfinite(b["scale"]).all()


@pytest.mark.parametrize("N,M,L,dtype", [(3000, 300, 3, torch.float32), (1500, 1100, 2, torch.float64)])
@pytest.mark.parametrize("kind", KINDS)
def test_blocked_factor_path_against_the_oracle(kind, N, M, L, dtype):
    """Beyond one 128-block (three blocks in fp32; nine, an odd count, in fp64): the whole forward against the oracle."""
    c, g, spec, extra = _problem(kind, N, M, L, 2, dtype)
    e, mean, scale = MO.elbo_eval(kind, c["whitened"], c["X"], c["y"], c["Z"], c["sigma"], c["lengthscale"], c["mu"],
                                  c["Lu_raw"], c["jitter"], c["noise_sd"])
    rt = rtol_for(dtype)
    for kw in ((dict(), dict(materialize_kzx=False), dict(narrow_tiles=True)) if dtype == torch.float32 else (dict(),)):
        out = _run(c, g, spec, extra, retain=0.0, **kw)
        torch.testing.assert_close(out["mean"].cpu(), mean, rtol=rt, atol=rt * float(mean.abs().max()))
        torch.testing.assert_close(out["scale"].cpu(), scale, rtol=rt, atol=0)
        assert float(out["elbo"]) == pytest.approx(float(e), rel=rt)


# ---------------------------------------------------------------- training
def test_training_follows_the_oracle_and_the_graphed_step():
    """Five fp64 Adam steps of gpzoo.utilities.train on GaussianLikelihood(WSVGP(batched_Matern52)), Z frozen, everything
    else trainable, the rsample noise fixed: the losses of the same five steps taken with torch on the CPU oracle, and of
    the step captured as a HIP graph."""
    import torch.distributions.normal as tdn
    from gpzoo.gp import WSVGP
    from gpzoo.kernels import batched_Matern52
    from gpzoo.likelihoods import GaussianLikelihood
    from gpzoo.utilities import train
    from oracle import svgp_oracle as O
    N, M, L, E, steps, lr, jitter = 400, 100, 2, 2, 5, 1e-2, 1e-2
    g = torch.Generator().manual_seed(31)
    X = (torch.rand(N, 2, generator=g, dtype=torch.float64) - 0.5) * 24
    y = torch.stack([torch.sin(X[:, 0] / 3), torch.cos(X[:, 1] / 4)]) + 0.1 * torch.randn(L, N, generator=g, dtype=torch.float64)
    Z = X[torch.randperm(N, generator=g)[:M]].clone()
    init = dict(mu=0.1 * torch.randn(L, M, generator=g, dtype=torch.float64),
                Lu=0.05 * torch.randn(L, M, M, generator=g, dtype=torch.float64),
                sigma=torch.tensor([1.0, 0.8], dtype=torch.float64), lengthscale=torch.tensor([2.5, 4.0], dtype=torch.float64),
                noise=torch.tensor(0.3).double())      # (the module's noise is an fp32 constant cast up)
    eps = torch.randn(E, L, N, generator=g, dtype=torch.float64)

    # the oracle's five steps (CPU)
    p = {k: v.clone().requires_grad_(True) for k, v in init.items()}
    order = ("mu", "Lu", "sigma", "lengthscale", "noise")
    opt = torch.optim.Adam([p[k] for k in order], lr=lr)
    ref = []
    for _ in range(steps):
        opt.zero_grad()
        q = MO.parts("matern52", True, X, Z, p["sigma"], p["lengthscale"], p["mu"], p["Lu"], jitter)
        F = q["mean"][None] + q["scale"][None] * eps
        pY = torch.distributions.Normal(F, torch.nn.functional.softplus(p["noise"]))
        loss = -(pY.log_prob(y).mean(dim=0).sum() - O.whitened_kl(p["mu"], q["Lu"]).sum())
        loss.backward()
        opt.step()
        ref.append(float(loss))
    assert ref[-1] < ref[0]

    def make():
        k = batched_Matern52()
        k.sigma, k.lengthscale = nn.Parameter(init["sigma"].clone()), nn.Parameter(init["lengthscale"].clone())
        gp = WSVGP(k, dim=2, M=M, jitter=jitter)
        gp.Z = nn.Parameter(Z.clone(), requires_grad=False)
        gp.mu, gp.Lu = nn.Parameter(init["mu"].clone()), nn.Parameter(init["Lu"].clone())
        model = GaussianLikelihood(gp, noise=0.3).double().cuda()
        params = [gp.mu, gp.Lu, gp.kernel.sigma, gp.kernel.lengthscale, model.noise]
        return model, torch.optim.Adam(params, lr=lr)

    eps_dev = eps.cuda()
    orig = tdn._standard_normal
    tdn._standard_normal = lambda shape, dtype, device: eps_dev
    try:
        runs = []
        for graph in (False, True):
            model, opt = make()
            runs.append(train(model, opt, X.cuda(), y.cuda(), torch.device("cuda"), steps=steps, E=E, graph=graph))
    finally:
        tdn._standard_normal = orig
    rt = rtol_for(torch.float64)
    torch.testing.assert_close(torch.tensor(runs[0], dtype=torch.float64), torch.tensor(ref, dtype=torch.float64), rtol=rt, atol=0)
    torch.testing.assert_close(torch.tensor(runs[1], dtype=torch.float64), torch.tensor(runs[0], dtype=torch.float64), rtol=rt, atol=0)
