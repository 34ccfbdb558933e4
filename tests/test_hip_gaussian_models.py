"""GPU: the Gaussian factor models -- ``RSF`` over WSVGP, SVGP and VNNGP, and ``FA`` -- through the fused
``expected_loglik`` against fp64 autograd of the closed form built in torch from the model's own q(F), the training loops,
and ``score``.  N = 65 spots, D = 7 genes, M = 16 inducing points, L = 3 factors."""
import pytest
import torch
import torch.nn as nn

import gaussian_cases as GC

pytestmark = pytest.mark.gpu

N, D, M, L = 65, 7, 16, 3
KINDS = ("WSVGP", "SVGP", "VNNGP", "FA")


def problem(n=N, seed=41, noise=0.3):
    """Positions and data drawn from the model: smooth factors (sines of the position), real loadings, an intercept."""
    g = torch.Generator().manual_seed(seed)
    X = (torch.rand(n, 2, generator=g) - 0.5) * 20
    F = torch.stack([torch.sin(0.3 * X[:, 0]), torch.cos(0.25 * X[:, 1]), torch.sin(0.2 * (X[:, 0] + X[:, 1]))])
    W = torch.randn(D, L, generator=g)
    b = 2.0 * torch.randn(D, generator=g)
    y = b[:, None] + W @ F + noise * torch.randn(D, n, generator=g)
    return X, y


def make(kind, X, y, seed=4):
    import gpzoo.gp as G
    import gpzoo.kernels as K
    import gpzoo.likelihoods as li
    torch.manual_seed(seed)
    if kind == "FA":
        prior = G.GaussianPrior(y, L=L)
        prior.mean = nn.Parameter(0.5 * torch.randn(L, y.shape[1]))
        prior.scale = nn.Parameter(0.3 * torch.rand(L, y.shape[1]))
        model = li.FA(prior, y, L=L)
    else:
        k = K.NSF_RBF(sigma=1.0, lengthscale=4.0, L=L)
        gp = G.VNNGP(k, dim=2, M=M, K=4, jitter=1e-2) if kind == "VNNGP" else getattr(G, kind)(k, dim=2, M=M, jitter=1e-2)
        gp.Z = nn.Parameter(X[:M].clone())
        gp.mu = nn.Parameter(0.3 * torch.randn(L, M))
        gp.Lu = nn.Parameter(0.05 * torch.randn(L, M, M) - 0.5 * torch.eye(M))
        model = li.RSF(gp, y, L=L)
    with torch.no_grad():                  # distinct noise levels per gene, so a gradient landing on the wrong gene shows
        model.noise.copy_(torch.linspace(-1.0, 1.5, D))
    return model.cuda()


def q_of(model, Xd):
    return model.prior()[0] if hasattr(model, "prior") else model.gp(Xd)[0]


def torch_closed_form(model, qF, yd):
    sd = torch.nn.functional.softplus(model.noise.double())
    return GC.closed_form(qF.mean.double(), qF.scale.double(), model.W.double(), model.b.double(), sd, yd.double())


@pytest.mark.parametrize("kind", KINDS)
def test_expected_loglik_equals_fp64_autograd_of_the_closed_form(kind):
    X, y = problem()
    model = make(kind, X, y)
    Xd, yd = X.cuda(), y.cuda()
    out = model.expected_loglik(Xd, yd, E=7)            # E is accepted and unused
    assert len(out) == (3 if kind == "FA" else 4)
    ll = out[0]
    assert ll.shape == () and ll.dtype == torch.float32
    ll.backward()
    got = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    missing = [n for n, p in model.named_parameters() if p.requires_grad and p.grad is None]
    assert not missing, missing
    model.zero_grad(set_to_none=True)
    want, _ = torch_closed_form(model, q_of(model, Xd), yd)
    want.backward()
    print(kind, "fused", float(ll), "torch fp64", float(want))
    assert float(ll) == pytest.approx(float(want), rel=5e-5, abs=1e-3)
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        sc = float(p.grad.abs().max()) + 1e-30
        err = float((got[n].double() - p.grad.double()).abs().max())
        print(f"  {n}: max err {err:.3e} of max |grad| {sc:.3e}")
        torch.testing.assert_close(got[n].double(), p.grad.double(), rtol=1e-3, atol=1e-3 * sc, msg=lambda m: f"{kind} {n}: {m}")
    assert {"W", "b", "noise"} <= set(got)


@pytest.mark.parametrize("whitened", [True, False])
def test_multi_group_gps_take_groupsX(whitened):
    """``groupsX=`` reaches the multi-group GPs as ``MGGP_NSF`` passes it (a keyword for MGGP_WSVGP, positional for
    MGGP_SVGP) and follows the sampled spots with ``idx``; ``train_batched`` runs with it."""
    import gpzoo.gp as G
    import gpzoo.kernels as K
    import gpzoo.likelihoods as li
    from gpzoo.utilities import train_batched
    X, y = problem()
    g = torch.Generator().manual_seed(6)
    gX = torch.randint(0, 3, (N,), generator=g)
    torch.manual_seed(4)
    k = K.MGGP_NSF_RBF(sigma=1.0, lengthscale=4.0, group_diff_param=0.8, n_groups=3, L=L)
    gp = G.MGGP_WSVGP(k, dim=2, M=M, n_groups=3, jitter=1e-2) if whitened else G.MGGP_SVGP(k, dim=2, M=M, jitter=1e-2, n_groups=3)
    gp.Z = nn.Parameter(X[:M].clone(), requires_grad=False)
    gp.groupsZ = nn.Parameter(gX[:M].clone(), requires_grad=False)
    gp.mu = nn.Parameter(0.3 * torch.randn(L, M))
    gp.Lu = nn.Parameter(0.05 * torch.randn(L, M, M) - 0.5 * torch.eye(M))
    model = li.RSF(gp, y, L=L).cuda()
    Xd, yd, gd = X.cuda(), y.cuda(), gX.cuda()
    ll, qF, qU, pU = model.expected_loglik(Xd, yd, groupsX=gd)
    want, _ = torch_closed_form(model, qF, yd)
    assert qF.mean.shape == (L, N) and float(ll) == pytest.approx(float(want), rel=5e-5, abs=1e-3)
    idx = torch.arange(3, 40).cuda()
    llb, qFb, _, _ = model.expected_loglik(Xd, yd[:, idx], idx=idx, groupsX=gd)
    torch.testing.assert_close(qFb.mean, qF.mean[:, idx], rtol=1e-4, atol=1e-5)
    wantb, _ = torch_closed_form(model, qFb, yd[:, idx])
    assert float(llb) == pytest.approx(float(wantb), rel=5e-5, abs=1e-3)
    s = model.score(Xd, yd[:, idx], idx=idx, groupsX=gd)
    assert float(s.loglik) == pytest.approx(float(wantb), rel=5e-5, abs=1e-3)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    losses = train_batched(model, opt, Xd, yd, steps=2, batch_size=32, groupsX=gd)
    assert len(losses) == 2 and all(v == v for v in losses)


def test_train_fused_and_graphed_agree():
    """``train`` on an RSF: the graphed loop follows the eager fused one (rtol 1e-4 over 10 steps, the figure of
    tests/test_hip_nb_models.py for the same comparison); the unfused loop, a Monte-Carlo estimate of the same
    objective, ends near it."""
    from gpzoo.utilities import train
    X, y = problem()
    Xd, yd = X.cuda(), y.cuda()
    runs = {}
    for name, kw in (("fused", dict(fused=True)), ("graph", dict(fused=True, graph=True))):
        model = make("WSVGP", X, y)
        opt = torch.optim.Adam(model.parameters(), lr=1e-2)
        torch.manual_seed(12)
        runs[name] = train(model, opt, Xd, yd, steps=10, E=3, **kw)
        assert bool((model.W < 0).any())
    print(runs)
    a, c = runs["fused"], runs["graph"]
    assert len(a) == len(c) == 10 and all(v == v for v in a + c)
    assert a[-1] < a[0]
    torch.testing.assert_close(torch.tensor(c), torch.tensor(a), rtol=1e-4, atol=0)


def test_train_batched_leaves_negative_loadings():
    from gpzoo.utilities import train_batched
    X, y = problem()
    model = make("WSVGP", X, y)
    assert bool((model.W < 0).any())
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    torch.manual_seed(13)
    losses = train_batched(model, opt, X.cuda(), y.cuda(), steps=3, E=3, batch_size=32, fused=True)
    assert len(losses) == 3 and all(v == v and abs(v) < float("inf") for v in losses)
    assert bool((model.W < 0).any())


def test_training_raises_held_out_r2():
    """Data drawn from the model, N = 400 with 10 % of the spots held out: 300 Adam steps bring the held-out R^2 above
    the untrained model's and above 0.  A direction check, not a fit-quality threshold."""
    from gpzoo.utilities import train
    X, y = problem(n=400, seed=43)
    g = torch.Generator().manual_seed(44)
    perm = torch.randperm(400, generator=g)
    held, fit = perm[:40], perm[40:]
    model = make("WSVGP", X[fit], y[:, fit])
    Xh, yh = X[held].cuda(), y[:, held].cuda()
    before = model.score(Xh, yh)
    opt = torch.optim.Adam(model.parameters(), lr=3e-2)
    torch.manual_seed(14)
    train(model, opt, X[fit].cuda(), y[:, fit].cuda(), steps=300, sync_losses=False)
    after = model.score(Xh, yh)
    print("held-out r2 before", float(before.r2), "after", float(after.r2), "loglik", float(before.loglik), float(after.loglik))
    assert float(after.r2) > float(before.r2) and float(after.r2) > 0.0


@pytest.mark.parametrize("kind", ["WSVGP", "FA"])
def test_score_agrees_with_torch_in_fp64(kind):
    """Every field to rtol 1e-5 with no absolute part.  ``r2`` = 1 - sse / null is an fp64 function of ``sse``, which is held
    to rtol 1e-5 here: that relative error in sse is an absolute error of 1e-5 sse / null in r2 (error propagation, no
    further slack), so r2 is held to 1e-5 (|r2| + sse / null) -- and to plain rtol 1e-5 wherever |r2| >= 0.1."""
    X, y = problem()
    y[3] = 1.25                                     # a constant gene: its R^2 is NaN, not a division by zero
    model = make(kind, X, y)
    Xd, yd = X.cuda(), y.cuda()
    idx = torch.arange(5, 50).cuda()
    s = model.score(Xd, yd[:, idx], idx=idx)
    assert all(t.dtype == torch.float64 and not t.requires_grad for t in s)
    with torch.no_grad():
        qF = model.prior.forward_batched(idx)[0] if kind == "FA" else model.gp(Xd[idx])[0]
        ll, sse = torch_closed_form(model, qF, yd[:, idx])
    B = idx.numel()
    yb = yd[:, idx].double()
    null = ((yb - yb.mean(1, keepdim=True)) ** 2).sum(1)
    assert float(null[3]) == 0.0
    kw = dict(rtol=1e-5, atol=0.0)
    torch.testing.assert_close(s.loglik, ll, **kw)
    torch.testing.assert_close(s.sse_per_gene, sse, **kw)
    torch.testing.assert_close(s.mse_per_gene, sse / B, **kw)
    torch.testing.assert_close(s.mse, sse.sum() / (D * B), **kw)
    keep = null > 0
    assert bool(torch.isnan(s.r2_per_gene[3])) and int(keep.sum()) == D - 1
    # r2 = 1 - sse / null: a relative error of 1e-5 in sse is an absolute one of 1e-5 sse / null in r2
    ratio, want = (sse / null)[keep], (1 - sse / null)[keep]
    assert bool(((s.r2_per_gene[keep] - want).abs() <= 1e-5 * (want.abs() + ratio)).all())
    big = want.abs() >= 0.1
    assert int(big.sum()) >= 1
    torch.testing.assert_close(s.r2_per_gene[keep][big], want[big], rtol=1e-5, atol=0.0)
    ratio, want = sse.sum() / null.sum(), 1 - sse.sum() / null.sum()
    assert float((s.r2 - want).abs()) <= 1e-5 * float(want.abs() + ratio)
    if float(want.abs()) >= 0.1:
        torch.testing.assert_close(s.r2, want, rtol=1e-5, atol=0.0)
