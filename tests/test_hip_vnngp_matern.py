"""GPU: VNNGP over the Matern family (nu = 1/2, 3/2, 5/2; ABI kinds 4, 1, 5), forward and backward, fp32 and fp64.

The module against the reference's own VNNGP run with these kernels (tests/golden/extra_vnngp_matern*.npz), everything
else against tests/vnngp_matern_oracle.py (tied to the same fixtures by tests/test_vnngp_matern.py) and torch autograd
through it.  References are computed once per parameter set (module-scoped caches) and left unchanged."""
import functools

import pytest
import torch
import torch.nn as nn

import vnngp_matern_oracle as VO
from helpers import load_case

pytestmark = pytest.mark.gpu

KINDS = VO.KINDS                                           # "matern12", "matern32", "matern52"
F64 = torch.float64


def _kind_id(kind):
    from gpzoo_amd import _lib
    return dict(matern12=_lib.KERNEL_MATERN12, matern32=_lib.KERNEL_MATERN32, matern52=_lib.KERNEL_MATERN52)[kind]


def _kernel_class(kind):
    import gpzoo.kernels as gk
    return dict(matern12=gk.batched_Matern12, matern32=gk.batched_Matern32, matern52=gk.batched_Matern52)[kind]


def _spec(kind, sigma, lengthscale):
    from gpzoo_amd.ops import KernelSpec
    return KernelSpec(_kind_id(kind), sigma.reshape(-1).cuda(), lengthscale.reshape(-1).cuda(), True)


def _close(got, ref, rt, name, at=None):
    """rtol = rt, atol = at max|ref|; ``at`` defaults to rt (the fixture and fp32 bars).  The fp64 comparisons with the
    oracle pass at = 1e-9: the bar test_hip_vnngp.py holds this pipeline to."""
    ref = ref.detach()
    torch.testing.assert_close(got.double().cpu().reshape(ref.shape), ref.double(), rtol=rt,
                               atol=(rt if at is None else at) * float(ref.abs().max()), msg=lambda m: f"{name}: {m}")


# ---- the module against the reference's fixtures -----------------------------------------------------------------------

def _module(c):
    from gpzoo.gp import VNNGP
    k = _kernel_class(c["kind"])()
    k.sigma = nn.Parameter(c["sigma"].clone()); k.lengthscale = nn.Parameter(c["lengthscale"].clone())
    gp = VNNGP(k, dim=2, M=c["Z"].shape[0], K=int(c["K"]), jitter=c["jitter"])
    gp.Z = nn.Parameter(c["Z"].clone()); gp.mu = nn.Parameter(c["mu"].clone()); gp.Lu = nn.Parameter(c["Lu_raw"].clone())
    return gp.cuda(), k


@functools.lru_cache(maxsize=None)
def _fixture_grad_Z(name):
    """The oracle's dLoss/dZ in fp64 on the fixture's inputs (the reference's own is NaN and is not stored)."""
    c = load_case(name)
    d = {k: c[k].double() for k in ("X", "y", "Z", "sigma", "lengthscale", "mu", "Lu_raw")}
    return VO.grads(c["kind"], d["X"], d["y"], d["Z"], d["sigma"], d["lengthscale"], d["mu"], d["Lu_raw"], c["jitter"],
                    int(c["K"]), c["noise_sd"], idx=c["idx"])["grad_Z"]


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_module_matches_reference(kind, tag):
    """ops.knn == idx; mean, scale, qU.scale_tril, pU.scale_tril as in test_hip_vnngp.py::test_module_matches_reference;
    loss and the gradients w.r.t. mu, Lu, sigma, lengthscale after loss.backward() against the reference's autograd with
    atol = rt max|ref|; grad_Z against the oracle's autograd at that bar."""
    from torch import distributions
    from gpzoo_amd import ops
    name = f"extra_vnngp_{kind}_{tag}"
    c = load_case(name)
    gp, k = _module(c)
    X, y, s = c["X"].cuda(), c["y"].cuda(), c["noise_sd"]
    assert torch.equal(ops.knn(X, gp.Z, int(c["K"])).cpu(), c["idx"])
    rt = 1e-5 if tag == "f64" else 1e-3
    with torch.no_grad():
        qF, qU, pU = gp(X)
    assert qF.mean.shape == c["mean"].shape
    torch.testing.assert_close(qF.mean.cpu(), c["mean"], rtol=rt, atol=rt * 1e-1)
    torch.testing.assert_close(qF.scale.cpu(), c["scale"], rtol=rt, atol=rt * 1e-1)
    torch.testing.assert_close(qU.scale_tril.cpu(), c["Lu"], rtol=rt, atol=rt * 1e-2)
    torch.testing.assert_close(pU.scale_tril.cpu(), c["chol"], rtol=rt, atol=rt * 1e-2)
    qF, qU, pU = gp(X)
    loss = -(distributions.Normal(qF.mean, s).log_prob(y).sum() - (qF.scale ** 2).sum() / (2 * s ** 2)
             - distributions.kl_divergence(qU, pU).sum())
    loss.backward()
    torch.testing.assert_close(float(loss.detach()), float(c["loss"]), rtol=rt, atol=0)
    for got, key in ((gp.mu.grad, "grad_mu"), (gp.Lu.grad, "grad_Lu"), (k.sigma.grad, "grad_sigma"),
                     (k.lengthscale.grad, "grad_lengthscale")):
        _close(got, c[key], rt, key)
    _close(gp.Z.grad, _fixture_grad_Z(name), rt, "grad_Z")


# ---- forward against the oracle, fp64 ----------------------------------------------------------------------------------

def _problem(seed, N, M, K, L, d, *, sig=(0.7, 1.0), lu_diag=0.0, lu=0.1, span=40.0, Z_from_X=False):
    g = torch.Generator().manual_seed(seed)
    X = (torch.rand(N, d, generator=g, dtype=F64) - 0.5) * span
    Z = X[torch.randperm(N, generator=g)[:M]].clone() if Z_from_X else (torch.rand(M, d, generator=g, dtype=F64) - 0.5) * span
    return dict(X=X, Z=Z, sigma=sig[0] + sig[1] * torch.rand(L, generator=g, dtype=F64),
                lengthscale=2.0 + 4 * torch.rand(L, generator=g, dtype=F64), mu=torch.randn(L, M, generator=g, dtype=F64),
                Lu=lu * torch.randn(L, M, M, generator=g, dtype=F64) + lu_diag * torch.eye(M, dtype=F64),
                a=torch.randn(L, N, generator=g, dtype=F64), b=torch.randn(L, N, generator=g, dtype=F64),
                gc=torch.randn(L, M, M, generator=g, dtype=F64).tril(), K=K)


# (N, M, K, L, d): K = 1, 5, 8 (KT = 8), 10 (KT = 12), 13, 16 (KT = 16), 17 and 32 (scratch form; 32: records of 98 values)
FWD_SHAPES = [(64, 5, 1, 1, 1), (257, 40, 5, 2, 2), (300, 33, 8, 3, 4), (3000, 60, 10, 4, 2), (500, 300, 13, 2, 2),
              (400, 129, 16, 1, 2), (333, 50, 17, 2, 1), (500, 40, 32, 2, 2)]


@pytest.mark.parametrize("shape", FWD_SHAPES, ids=lambda s: "N{}-M{}-K{}-L{}-d{}".format(*s))
@pytest.mark.parametrize("kind", KINDS)
def test_forward_against_oracle(kind, shape):
    from gpzoo_amd import ops
    N, M, K, L, d = shape
    p = _problem(N + K, N, M, K, L, d)
    mean, scale, idx, _, chol = VO.vnngp_moments(kind, p["X"], p["Z"], p["sigma"], p["lengthscale"], p["mu"], p["Lu"], 1e-2, K)
    out = ops.vnngp_forward(_spec(kind, p["sigma"], p["lengthscale"]), p["X"].cuda(), p["Z"].cuda(), p["mu"].cuda(),
                            p["Lu"].cuda(), 1e-2, K)
    assert torch.equal(out["idx"].cpu(), idx)
    torch.testing.assert_close(out["mean"].cpu(), mean, rtol=1e-7, atol=1e-9)
    torch.testing.assert_close(out["scale"].cpu(), scale, rtol=1e-7, atol=1e-9)
    torch.testing.assert_close(out["chol"].cpu(), chol.reshape(L, M, M), rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize("kind", KINDS)
def test_scalar_parameter_kernel_through_the_module(kind):
    """Scalar sigma / lengthscale with (M,) mu and (M,M) Lu: (N,) moments, as scalar RBF gives."""
    from gpzoo.gp import VNNGP
    N, M, K = 300, 33, 7
    p = _problem(11, N, M, K, 1, 2)
    gp = VNNGP(_kernel_class(kind)(sigma=0.875, lengthscale=3.0), dim=2, M=M, K=K, jitter=1e-2).double()
    gp.Z = nn.Parameter(p["Z"].clone()); gp.mu = nn.Parameter(p["mu"][0].clone()); gp.Lu = nn.Parameter(p["Lu"][0].clone())
    gp = gp.cuda()
    s, ell = torch.tensor(0.875, dtype=F64), torch.tensor(3.0, dtype=F64)
    mean, scale, _, Lu, chol = VO.vnngp_moments(kind, p["X"], p["Z"], s, ell, p["mu"][0], p["Lu"][0], 1e-2, K)
    with torch.no_grad():
        qF, qU, pU = gp(p["X"].cuda())
    assert qF.mean.shape == (N,) and qF.scale.shape == (N,) and pU.scale_tril.shape == (M, M)
    torch.testing.assert_close(qF.mean.cpu(), mean, rtol=1e-7, atol=1e-9)
    torch.testing.assert_close(qF.scale.cpu(), scale, rtol=1e-7, atol=1e-9)
    torch.testing.assert_close(qU.scale_tril.cpu(), Lu, rtol=1e-7, atol=1e-9)
    torch.testing.assert_close(pU.scale_tril.cpu(), chol, rtol=1e-7, atol=1e-9)


# ---- backward against the oracle's autograd ----------------------------------------------------------------------------

def _table(p, dup):
    """The fp64 argsort table; ``dup``: with repeated neighbours as in test_caller_table_with_repeated_neighbours."""
    K = p["K"]
    idx = torch.argsort(torch.cdist(p["X"], p["Z"]), dim=1)[:, :K].clone()
    if dup:
        idx[::3, K - 1] = idx[::3, 0]
        idx[1::7, 4] = idx[1::7, 2]; idx[1::7, 6] = idx[1::7, 2]
        idx[5::11, :] = idx[5::11, :1]
    return idx


def _reference(kind, p, idx, with_chol=True):
    """Oracle moments and the autograd gradients of sum(a mean) + sum(b scale) [+ sum(gc chol)]."""
    leaf = {n: p[n].detach().clone().requires_grad_(True) for n in ("Z", "sigma", "lengthscale", "mu", "Lu")}
    mean, scale, _, _, chol, cov = VO.vnngp_moments(kind, p["X"], leaf["Z"], leaf["sigma"], leaf["lengthscale"], leaf["mu"],
                                                    leaf["Lu"], 1e-2, p["K"], idx=idx, with_cov=True)
    loss = (p["a"] * mean).sum() + (p["b"] * scale).sum()
    if with_chol:
        loss = loss + (p["gc"] * chol.reshape(p["gc"].shape)).sum()
    loss.backward()
    return dict(mean=mean.detach(), scale=scale.detach(), cov=cov.detach(), **{n: t.grad for n, t in leaf.items()})


def _round(p, dtype):
    """The problem with every floating-point input rounded to ``dtype`` (values kept in fp64)."""
    return {k: (v.to(dtype).double() if torch.is_tensor(v) else v) for k, v in p.items()}


def _run(kind, p, idx, dtype=F64, frozen=False, with_chol=True, forward=False, **kw):
    from gpzoo_amd import ops
    c = lambda t: t.detach().to(dtype).cuda()      # noqa: E731
    spec = _spec(kind, c(p["sigma"]), c(p["lengthscale"]))
    args = (spec, c(p["X"]), c(p["Z"]), c(p["mu"]), c(p["Lu"]), 1e-2, p["K"])
    res = ops.vnngp_backward(*args, idx.cuda(), c(p["a"]), c(p["b"]), kernel_grads=not frozen,
                             g_chol=c(p["gc"]) if (with_chol and not frozen) else None, **kw)
    if forward:
        return res, ops.vnngp_forward(*args, idx=idx.cuda())
    return res


def _check_grads(res, ref, rt, frozen=False):
    """fp64 (rt = 1e-7): rtol 1e-7, atol 1e-9 max|ref|; fp32 (rt = 1e-3): rtol 1e-3, atol 1e-3 max|ref|."""
    at = 1e-9 if rt <= 1e-7 else rt
    _close(res[0], ref["mu"], rt, "grad_mu", at); _close(res[1], ref["Lu"], rt, "grad_Lu", at)
    if not frozen:
        _close(res[2][:, 0], ref["sigma"], rt, "grad_sigma", at)
        _close(res[2][:, 1], ref["lengthscale"], rt, "grad_lengthscale", at)
        _close(res[3], ref["Z"], rt, "grad_Z", at)


BWD_PROBLEMS = dict(
    clamped=dict(seed=77, N=2000, M=200, K=8, L=3, d=2, sig=(0.25, 0.2), lu=0.05, lu_diag=-1.5, span=30.0),   # the existing recipe
    k20=dict(seed=20, N=600, M=60, K=20, L=2, d=2, span=30.0),                   # scratch-form backward
    k24=dict(seed=24, N=500, M=48, K=24, L=2, d=3, span=20.0),                   # records of 74 values: two loads per entry
    k13=dict(seed=13, N=700, M=130, K=13, L=3, d=1, span=60.0),                  # KT = 16 backward, more than one 128-block
    zero=dict(seed=5, N=300, M=40, K=6, L=2, d=2, span=30.0, Z_from_X=True),     # Z = rows of X: r = 0 in k_xz
    f32=dict(seed=32, N=1500, M=120, K=9, L=2, d=2, sig=(0.6, 0.3), lu=0.05, lu_diag=-1.0, span=30.0),
)


@functools.lru_cache(maxsize=None)
def _bwd_case(kind, which, dtype=F64, dup=False):
    p = _round(_problem(**BWD_PROBLEMS[which]), dtype)
    idx = _table(p, dup)
    return p, idx, _reference(kind, p, idx)


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_backward_with_clamped_points(kind, frozen):
    """A strict subset of the variances at the 5e-2 clamp (no gradient through those); ``frozen``: no kernel / Z gradients."""
    p, idx, ref = _bwd_case(kind, "clamped")
    n_clamped = int((ref["scale"] ** 2 <= 5e-2 * (1 + 1e-9)).sum())
    assert 0 < n_clamped < ref["scale"].numel()
    if frozen:                                # the oracle's loss carries the chol term; mu and Lu do not see it
        res = _run(kind, p, idx, frozen=True)
        assert len(res) == 2
        _check_grads(res, ref, 1e-7, frozen=True)
    else:
        _check_grads(_run(kind, p, idx), ref, 1e-7)


@pytest.mark.parametrize("which", ["k20", "k24", "k13"])
@pytest.mark.parametrize("kind", KINDS)
def test_backward_against_oracle_autograd(kind, which):
    p, idx, ref = _bwd_case(kind, which)
    res, out = _run(kind, p, idx, forward=True)
    torch.testing.assert_close(out["mean"].cpu(), ref["mean"], rtol=1e-7, atol=1e-9)
    torch.testing.assert_close(out["scale"].cpu(), ref["scale"], rtol=1e-7, atol=1e-9)
    _check_grads(res, ref, 1e-7)


@pytest.mark.parametrize("kind", KINDS)
def test_zero_distance(kind):
    """Every inducing point is a datum: r = 0 in k_xz for those points (and on Kzz's diagonal).  Every output and gradient
    finite and equal to the oracle's, whose masked square root gives dk/dz = 0 at r = 0 -- for nu = 1/2 a convention."""
    p, idx, ref = _bwd_case(kind, "zero")
    d2 = ((p["X"][:, None, :] - p["Z"][None, :, :]) ** 2).sum(-1)
    assert int((d2 == 0).sum()) == p["Z"].shape[0] and bool((d2.gather(1, idx)[:, 0] == d2.min(dim=1).values).all())
    res, out = _run(kind, p, idx, forward=True)
    for t in (out["mean"], out["scale"], *res):
        assert bool(torch.isfinite(t).all())
    torch.testing.assert_close(out["mean"].cpu(), ref["mean"], rtol=1e-7, atol=1e-9)
    torch.testing.assert_close(out["scale"].cpu(), ref["scale"], rtol=1e-7, atol=1e-9)
    _check_grads(res, ref, 1e-7)
    # and in fp32, at the fp32 bar against the fp64 oracle on the fp32-rounded inputs
    p32, idx32, ref32 = _bwd_case(kind, "zero", torch.float32)
    res32 = _run(kind, p32, idx32, torch.float32)
    assert all(bool(torch.isfinite(t).all()) for t in res32)
    _check_grads(res32, ref32, 1e-3)


@pytest.mark.parametrize("dup", [False, True], ids=["distinct", "repeated"])
@pytest.mark.parametrize("kind", KINDS)
def test_backward_fp32(kind, dup):
    """fp32 against the fp64 oracle on the same fp32-rounded inputs; ``repeated``: a caller-supplied table that names an
    inducing point twice, three times and K times (the gather then adds lane after lane)."""
    p, idx, ref = _bwd_case(kind, "f32", torch.float32, dup)
    res, out = _run(kind, p, idx, torch.float32, with_chol=True, forward=True)
    _close(out["mean"], ref["mean"], 1e-3, "mean"); _close(out["scale"], ref["scale"], 1e-3, "scale")
    _check_grads(res, ref, 1e-3)
    again = _run(kind, p, idx, torch.float32)
    assert all(torch.equal(x, y) for x, y in zip(res, again))


# ---- bitwise reproducibility -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_bitwise_reproducible(kind, dtype):
    """Forward twice, backward twice: equal bits.  With the forward's handed-over state: equal bits.  With ``point_order``
    (Morton, and an arbitrary permutation) the same sums are formed in another fixed order: equal bits from run to run and
    equal to the unordered result to rounding -- a reordered sum cannot keep its bits (bounds as in
    test_hip_vnngp.py::test_backward_with_handed_over_state_and_point_order)."""
    from gpzoo_amd import ops
    N, M, K, L = 1500, 100, 10, 2
    p = _problem(31, N, M, K, L, 2, sig=(0.6, 0.3), lu=0.05, lu_diag=-1.0, span=60.0)
    c = lambda t: t.to(dtype).cuda()      # noqa: E731
    spec = _spec(kind, c(p["sigma"]), c(p["lengthscale"]))
    args = (spec, c(p["X"]), c(p["Z"]), c(p["mu"]), c(p["Lu"]), 1e-2, K)
    gkl = torch.ones(L, dtype=F64).cuda()
    f1, f2 = ops.vnngp_forward(*args), ops.vnngp_forward(*args)
    for key in ("mean", "scale", "chol", "Lu", "kl", "idx"):
        assert torch.equal(f1[key], f2[key]), key

    def run(with_state, order):
        out = ops.vnngp_forward(*args, keep_state=with_state)
        return ops.vnngp_backward(*args, out["idx"], c(p["a"]), c(p["b"]), kernel_grads=True, g_kl=gkl,
                                  state=out.get("state"), point_order=order)
    base = run(False, None)
    for other in (run(False, None), run(True, None)):
        assert all(torch.equal(x, y) for x, y in zip(base, other))
    rt = 1e-10 if dtype == F64 else 2e-4
    for order in (ops.morton_order(args[1]), torch.randperm(N, generator=torch.Generator().manual_seed(1)).cuda()):
        r1, r2 = run(True, order), run(True, order)
        for x, y, z in zip(base, r1, r2):
            assert torch.equal(y, z)
            torch.testing.assert_close(y, x, rtol=rt, atol=rt * float(x.abs().max()))


@pytest.mark.parametrize("dtype", [F64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_backward_with_a_hub_is_bitwise_reproducible(kind, dtype):
    """The hub-point recipe of test_hip_vnngp.py::test_backward_is_bitwise_reproducible: an inducing point every datum names."""
    from gpzoo_amd import ops
    N, M, K, L = 2500, 150, 8, 2
    p = _problem(2024, N, M, K, L, 2, sig=(0.5, 0.2), lu=0.05, lu_diag=-1.5, span=30.0)
    c = lambda t: t.to(dtype).cuda()      # noqa: E731
    spec = _spec(kind, c(p["sigma"]), c(p["lengthscale"]))
    idx = ops.knn(c(p["X"]), c(p["Z"]), K)
    for hub in (7, 8, 9):                           # the last slot names the hub unless the datum holds it already
        free = ~(idx[:, : K - 1] == hub).any(1)
        if hub == 7:
            idx[free, K - 1] = hub
            todo = ~free
        else:
            idx[todo & free, K - 1] = hub
            todo = todo & ~free
    assert bool((idx.sort(dim=1).values.diff(dim=1) != 0).all())       # every datum's neighbours stay distinct
    assert int((idx == 7).sum()) == N
    runs = [ops.vnngp_backward(spec, c(p["X"]), c(p["Z"]), c(p["mu"]), c(p["Lu"]), 1e-2, K, idx, c(p["a"]), c(p["b"]),
                               kernel_grads=True) for _ in range(3)]
    for r in runs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(runs[0], r))
    assert all(bool(torch.isfinite(t).all()) for t in runs[0])


@pytest.mark.parametrize("kind", KINDS)
def test_module_backward_twice_gives_equal_bits(kind):
    from torch import distributions
    c = load_case(f"extra_vnngp_{kind}_f32")
    X, y = c["X"].cuda(), c["y"].cuda()
    grads = []
    for _ in range(2):
        gp, k = _module(c)
        qF, qU, pU = gp(X)
        loss = -(distributions.Normal(qF.mean, 0.5).log_prob(y).sum() - (qF.scale ** 2).sum() / 0.5
                 - distributions.kl_divergence(qU, pU).sum())
        loss.backward()
        grads.append([loss.detach()] + [t.grad for t in (gp.mu, gp.Lu, gp.Z, k.sigma, k.lengthscale)])
    assert all(torch.equal(x, y) for x, y in zip(*grads))


# ---- training, and what stays refused ----------------------------------------------------------------------------------

def _training_model(kernel):
    from gpzoo.gp import VNNGP
    from gpzoo.likelihoods import GaussianLikelihood
    g = torch.Generator().manual_seed(9)
    N, M = 400, 60
    X = (torch.rand(N, 2, generator=g) - 0.5) * 20
    y = torch.sin(X[:, 0] / 3.0) + 0.1 * torch.randn(N, generator=g)
    gp = VNNGP(kernel, dim=2, M=M, K=8, jitter=1e-2)
    gp.Z = nn.Parameter(X[torch.randperm(N, generator=g)[:M]].clone())
    gp.Lu = nn.Parameter(0.05 * torch.randn(M, M, generator=g) - 1.0 * torch.eye(M))
    return GaussianLikelihood(gp, noise=0.5).cuda(), X.cuda(), y.cuda()


def test_vnngp_matern32_trains_and_refuses_a_user_defined_covariance():
    """VNNGP(batched_Matern32) under GaussianLikelihood through utilities.train: finite losses, lower at the end.  The
    same model with a user-overridden ``covariance`` raises instead of being evaluated with the closed form."""
    import math
    from gpzoo.kernels import batched_Matern32
    from gpzoo.utilities import train
    model, X, y = _training_model(batched_Matern32(sigma=1.0, lengthscale=3.0))
    torch.manual_seed(0)
    losses = train(model, torch.optim.Adam(model.parameters(), lr=2e-2), X, y, steps=40, E=10)
    assert len(losses) == 40 and all(math.isfinite(v) for v in losses)
    assert losses[-1] < losses[0]
    assert all(p.grad is not None for p in model.parameters())

    class Mine(batched_Matern32):
        def covariance(self, x1, x2):
            return (self.sigma ** 2) * torch.exp(-((x1 - x2) ** 2).sum() / self.lengthscale)

    model, X, y = _training_model(Mine(sigma=1.0, lengthscale=3.0))
    with pytest.raises(NotImplementedError, match="user-defined"):
        model.gp(X)
    with pytest.raises(NotImplementedError, match="user-defined"):
        train(model, torch.optim.Adam(model.parameters(), lr=1e-2), X, y, steps=1, E=2)


def test_multi_group_kernel_is_still_refused():
    from gpzoo_amd import _lib, ops
    from gpzoo_amd.ops import KernelSpec
    p = _problem(3, 64, 12, 4, 2, 2)
    spec = KernelSpec(_lib.KERNEL_MGGP_RBF, p["sigma"].cuda(), p["lengthscale"].cuda(), True,
                      torch.ones(2, dtype=F64).cuda(), torch.zeros(2, 2, dtype=F64).cuda(), 1.0)
    args = (spec, p["X"].cuda(), p["Z"].cuda(), p["mu"].cuda(), p["Lu"].cuda(), 1e-2, 4)
    with pytest.raises(RuntimeError, match=r"gpz_vnngp: kernel kind 2 \(multi-group"):      # vnn_check's own message
        ops.vnngp_forward(*args)
    idx = torch.zeros(64, 4, dtype=torch.int64).cuda()
    with pytest.raises(RuntimeError, match=r"gpz_vnngp: kernel kind 2 \(multi-group"):
        ops.vnngp_backward(*args, idx, p["a"].cuda(), p["b"].cuda(), kernel_grads=True)
