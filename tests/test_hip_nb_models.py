"""GPU: the count models with ``likelihood="nb"`` -- the fused ``expected_loglik`` against the models' own unfused
``forward`` (torch's NegativeBinomial over the (E, D, N) rate) in value and in every parameter's gradient, the training
loops (fused, unfused, graphed) on an NB model, and the direction theta moves on overdispersed data.
Two spatial factors and one non-spatial one; N = 200 spots, D = 30 genes, M = 40 inducing points."""
import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

N, D, M, L, T, E, GROUPS = 200, 30, 40, 2, 1, 3, 3
KINDS = ("NSF", "NSF2", "Hybrid_NSF2", "MGGP_NSF")


def problem(seed=21, theta=2.0):
    """Positions, group ids and gamma-Poisson counts with the given inverse dispersion for every gene."""
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    X = (torch.rand(N, 2, generator=g) - 0.5) * 20
    gX = torch.randint(0, GROUPS, (N,), generator=g)
    rate = 0.5 + 4.0 * rng.random((D, 1)) * (0.3 + rng.random((1, N)))
    y = torch.from_numpy(rng.poisson(rng.gamma(theta, rate / theta)).astype(np.float32))
    return X, gX, y


def make(kind, X, gX, y, likelihood="nb", theta0=10.0, seed=4, spread_theta=True):
    import gpzoo.gp as G
    import gpzoo.kernels as K
    import gpzoo.likelihoods as li
    torch.manual_seed(seed)
    if kind == "MGGP_NSF":
        k = K.MGGP_NSF_RBF(sigma=1.0, lengthscale=4.0, group_diff_param=0.8, n_groups=GROUPS, L=L)
        gp = G.MGGP_WSVGP(k, dim=2, M=M, n_groups=GROUPS, jitter=1e-2)
        gp.groupsZ = nn.Parameter(gX[:M].clone(), requires_grad=False)
    else:
        gp = G.WSVGP(K.NSF_RBF(sigma=1.0, lengthscale=4.0, L=L), dim=2, M=M, jitter=1e-2)
    gp.Z = nn.Parameter(X[:M].clone(), requires_grad=False)
    gp.mu = nn.Parameter(0.1 * torch.randn(L, M))
    gp.Lu = nn.Parameter(0.05 * torch.randn(L, M, M) - 0.5 * torch.eye(M))
    kw = dict(likelihood=likelihood, theta0=theta0)
    if kind == "Hybrid_NSF2":
        model = li.Hybrid_NSF2(gp, G.GaussianPrior(y, L=T), y, L=L, T=T, **kw)
    else:
        model = getattr(li, kind)(gp, y, L=L, **kw)
    if likelihood == "nb" and spread_theta:      # distinct dispersions per gene, so a gradient landing on the wrong gene shows
        with torch.no_grad():
            model.theta.copy_(torch.linspace(0.5, 6.0, D))
    return model.cuda()


def replay(eps_list):
    """Patch for torch.distributions.normal._standard_normal that hands out the given draws in order."""
    queue = list(eps_list)
    return lambda shape, dtype, device: queue.pop(0).to(dtype)


@pytest.mark.parametrize("kind", KINDS)
def test_expected_loglik_equals_the_unfused_forward(kind):
    import torch.distributions.normal as tdn
    X, gX, y = problem()
    model = make(kind, X, gX, y)
    Xd, gd, yd = X.cuda(), gX.cuda(), y.cuda()
    g = torch.Generator().manual_seed(8)
    eps = [torch.randn(E, L, N, generator=g).cuda()] + ([torch.randn(E, T, N, generator=g).cuda()] if kind == "Hybrid_NSF2" else [])
    extra = dict(groupsX=gd) if kind == "MGGP_NSF" else {}
    # fused, fp32
    ll = model.expected_loglik(Xd, yd, E=E, eps=torch.cat(eps, dim=1), **extra)[0]
    ll.backward()
    # unfused: the model's own forward, in fp64, with the same draws
    ref = make(kind, X, gX, y).double()          # the same seed: the same initial parameters
    for (na, a), (nb, b) in zip(model.named_parameters(), ref.named_parameters()):
        assert na == nb and torch.equal(a.detach().double(), b.detach()), na
    orig = tdn._standard_normal
    try:
        tdn._standard_normal = replay(eps)
        with torch.no_grad():
            pY32 = (model(Xd, gd, E=E) if kind == "MGGP_NSF" else model(X=Xd, E=E))[0]
        tdn._standard_normal = replay(eps)
        pY = (ref(Xd.double(), gd, E=E) if kind == "MGGP_NSF" else ref(X=Xd.double(), E=E))[0]
    finally:
        tdn._standard_normal = orig
    assert isinstance(pY, torch.distributions.NegativeBinomial) and pY.logits.shape == (E, D, N)
    with torch.no_grad():
        ll32 = float(pY32.log_prob(yd).mean(0).sum())
    want = pY.log_prob(yd.double()).mean(0).sum()
    want.backward()
    print(kind, "fused", float(ll), "forward fp32", ll32, "forward fp64", float(want))
    assert float(ll) == pytest.approx(float(want), rel=5e-5, abs=1e-3)
    assert ll32 == pytest.approx(float(want), rel=5e-4)            # the fp32 torch evaluation itself
    got = dict(model.named_parameters())
    seen = set()
    for name, p in ref.named_parameters():
        if p.grad is None:
            continue
        seen.add(name.split(".")[-1])
        assert got[name].grad is not None, name
        sc = float(p.grad.abs().max()) + 1e-30
        err = float((got[name].grad.double() - p.grad).abs().max())
        print(f"  {name}: max err {err:.3e} of max |grad| {sc:.3e}")
        torch.testing.assert_close(got[name].grad.double(), p.grad, rtol=1e-3, atol=1e-3 * sc, msg=lambda m: f"{kind} {name}: {m}")
    assert {"theta", "W", "V", "mu", "Lu"} <= seen


def test_training_loops_take_an_nb_model():
    """train with fused=True and fused=False from the same seed agree loss by loss to 2e-3 relative (the bound of the
    Poisson loops' comparison in tests/test_hip_poisson.py); the graphed loop follows the eager fused one (Adam's
    capturable form rounds its bias corrections differently: 1e-4 relative in fp32 over a dozen steps)."""
    from gpzoo.utilities import train
    X, gX, y = problem()
    Xd, yd = X.cuda(), y.cuda()
    runs = {}
    for name, kw in (("fused", dict(fused=True)), ("unfused", dict(fused=False)), ("graph", dict(fused=True, graph=True))):
        model = make("NSF", X, gX, y)
        opt = torch.optim.Adam(model.parameters(), lr=1e-2)
        torch.manual_seed(12)
        runs[name] = train(model, opt, Xd, yd, steps=12, E=3, **kw)
        assert model.theta.grad is not None or name == "graph"
    print(runs)
    a, b, c = runs["fused"], runs["unfused"], runs["graph"]
    assert len(a) == len(b) == len(c) == 12 and all(v == v for v in a + b + c)
    assert all(abs(u - v) <= 2e-3 * abs(v) for u, v in zip(a, b)), (a, b)
    torch.testing.assert_close(torch.tensor(c), torch.tensor(a), rtol=1e-4, atol=0)


@pytest.mark.parametrize("loop", ["train_batched", "train_hybrid", "train_hybrid_batched"])
def test_minibatch_and_hybrid_loops_take_an_nb_model(loop):
    import gpzoo.utilities as U
    X, gX, y = problem()
    kind = "NSF" if loop == "train_batched" else "Hybrid_NSF2"
    model = make(kind, X, gX, y)
    before = model.theta.detach().clone()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    torch.manual_seed(13)
    kw = dict(batch_size=64) if "batched" in loop else {}
    losses = getattr(U, loop)(model, opt, X.cuda(), y.cuda(), steps=3, E=3, fused=True, **kw)
    assert len(losses) == 3 and all(v == v and abs(v) < float("inf") for v in losses)
    assert not torch.equal(model.theta.detach(), before)


def test_theta_moves_towards_the_overdispersion_of_the_data():
    """Counts with theta = 2 for every gene: 200 Adam steps move the median fitted theta down from theta0 = 10, and the NB
    model's loss ends below the Poisson model's on the same data, the latter evaluated as an NB log-likelihood at
    theta = 1e4.  A direction check, not a fit-quality threshold."""
    import torch.nn.functional as Fn
    from gpzoo.likelihoods import nb_expected_loglik
    from gpzoo.utilities import train
    from gpzoo_amd.utilities import _kl_u
    X, gX, y = problem(seed=33, theta=2.0)
    Xd, yd = X.cuda(), y.cuda()
    models = {}
    for lik in ("nb", "poisson"):
        model = make("NSF", X, gX, y, likelihood=lik, theta0=10.0, seed=3, spread_theta=False)
        opt = torch.optim.Adam(model.parameters(), lr=2e-2)
        torch.manual_seed(14)
        train(model, opt, Xd, yd, steps=200, E=3, sync_losses=False)
        models[lik] = model
    theta = Fn.softplus(models["nb"].theta.detach())
    g = torch.Generator().manual_seed(15)
    eps = torch.randn(8, L, N, generator=g).cuda()
    loss = {}
    with torch.no_grad():
        for lik, m in models.items():
            qF, qU, pU = m.gp(X=Xd)
            th = theta if lik == "nb" else torch.full((D,), 1e4, device="cuda")
            ll = nb_expected_loglik([qF], [Fn.softplus(m.W)], Fn.softplus(m.V), th, yd, eps=eps)
            loss[lik] = float(-(ll - _kl_u(qU, pU)))
    print("median theta", float(theta.median()), "losses", loss)
    assert float(theta.median()) < 10.0
    assert loss["nb"] < loss["poisson"]
