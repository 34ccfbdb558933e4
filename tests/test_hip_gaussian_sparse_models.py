"""GPU: ``RSF`` and ``FA`` on a ``SparseExpression`` -- ``expected_loglik`` with ``.backward()``, ``score`` and the training
loops -- against the same model on the dense array ``expr.to_dense()``.  N = 130 spots, D = 40 genes, M = 16 inducing
points, L = 4 factors; the expression is ``log_normalize`` of thinned Poisson counts."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

N, D, M, L = 130, 40, 16, 4


def problem(seed=51):
    """Positions, counts drawn from smooth non-negative factors and thinned to about a third, and their normalisation."""
    import gpzoo.likelihoods as li
    from gpzoo.utilities import log_normalize
    g = torch.Generator().manual_seed(seed)
    X = (torch.rand(N, 2, generator=g) - 0.5) * 20
    F = torch.stack([torch.sin(0.3 * X[:, 0]), torch.cos(0.25 * X[:, 1]), torch.sin(0.2 * (X[:, 0] + X[:, 1])),
                     torch.cos(0.15 * (X[:, 0] - X[:, 1]))])
    rate = torch.exp(0.5 * torch.rand(D, L, generator=g) @ F + 0.8)
    y = torch.poisson(rate, generator=g) * (torch.rand(D, N, generator=g) < 0.35)
    y[7] = 0.0                                      # a gene without counts: constant after centring, its R^2 is NaN
    expr = log_normalize(li.SparseCounts(y))
    return X, expr


def make(kind, X, y, seed=4):
    import gpzoo.gp as G
    import gpzoo.kernels as K
    import gpzoo.likelihoods as li
    torch.manual_seed(seed)
    if kind == "FA":
        prior = G.GaussianPrior(torch.zeros(D, N), L=L)
        prior.mean = nn.Parameter(0.5 * torch.randn(L, N))
        prior.scale = nn.Parameter(0.3 * torch.rand(L, N))
        model = li.FA(prior, y, L=L)
    else:
        gp = G.WSVGP(K.NSF_RBF(sigma=1.0, lengthscale=4.0, L=L), dim=2, M=M, jitter=1e-2)
        gp.Z = nn.Parameter(X[:M].clone())
        gp.mu = nn.Parameter(0.3 * torch.randn(L, M))
        gp.Lu = nn.Parameter(0.05 * torch.randn(L, M, M) - 0.5 * torch.eye(M))
        model = li.RSF(gp, y, L=L)
    with torch.no_grad():                  # distinct noise levels per gene, so a gradient landing on the wrong gene shows
        model.noise.copy_(torch.linspace(-1.0, 1.5, D))
    return model.cuda()


def pair(kind, X, expr):
    """The model built from the SparseExpression and the one built from its dense array, with the same parameters."""
    sparse, dense = make(kind, X, expr), make(kind, X, expr.to_dense())
    for (n1, p1), (n2, p2) in zip(sparse.named_parameters(), dense.named_parameters()):
        assert n1 == n2
        torch.testing.assert_close(p1, p2, rtol=0, atol=1e-6)          # b and noise come from segment sums / from the array
    dense.load_state_dict(sparse.state_dict())
    return sparse, dense


@pytest.mark.parametrize("kind,batch", [("WSVGP", False), ("WSVGP", True), ("FA", False), ("FA", True)])
def test_expected_loglik_and_gradients_match_the_dense_model(kind, batch):
    X, expr = problem()
    sparse, dense = pair(kind, X, expr)
    Xd, ed = X.cuda(), expr.cuda()
    yd = ed.to_dense()
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(3))[:50].cuda() if batch else None
    out = sparse.expected_loglik(Xd, ed if idx is None else ed[:, idx], idx=idx)
    ref = dense.expected_loglik(Xd, yd if idx is None else yd[:, idx], idx=idx)
    assert len(out) == len(ref) == (3 if kind == "FA" else 4)
    assert out[0].shape == () and out[0].dtype == torch.float32
    out[0].backward()
    ref[0].backward()
    print(kind, "batch" if batch else "full", "sparse", float(out[0]), "dense", float(ref[0]))
    assert float(out[0]) == pytest.approx(float(ref[0]), rel=1e-3)
    names = [n for n, p in dense.named_parameters() if p.requires_grad]
    assert {"W", "b", "noise"} <= set(names)
    for (n, p), (_, q) in zip(sparse.named_parameters(), dense.named_parameters()):
        if not q.requires_grad:
            continue
        assert p.grad is not None, n
        sc = float(q.grad.abs().max()) + 1e-30
        err = float((p.grad.double() - q.grad.double()).abs().max())
        print(f"  {n}: max err {err:.3e} of max |grad| {sc:.3e}")
        torch.testing.assert_close(p.grad.double(), q.grad.double(), rtol=1e-3, atol=1e-3 * sc, msg=lambda m: f"{kind} {n}: {m}")


@pytest.mark.parametrize("kind", ["WSVGP", "FA"])
def test_score_matches_the_dense_score(kind):
    X, expr = problem()
    sparse, dense = pair(kind, X, expr)
    Xd, ed = X.cuda(), expr.cuda()
    yd = ed.to_dense()
    idx = torch.arange(5, 95).cuda()
    for view in (False, True):
        s = sparse.score(Xd, ed[:, idx] if view else ed, idx=idx if view else None)
        r = dense.score(Xd, yd[:, idx] if view else yd, idx=idx if view else None)
        assert all(t.dtype == torch.float64 and not t.requires_grad for t in s)
        kw = dict(rtol=1e-5, atol=0.0)
        torch.testing.assert_close(s.sse_per_gene, r.sse_per_gene, **kw)
        torch.testing.assert_close(s.mse_per_gene, r.mse_per_gene, **kw)
        torch.testing.assert_close(s.mse, r.mse, **kw)
        torch.testing.assert_close(s.loglik, r.loglik, **kw)
        assert bool(torch.isnan(s.r2_per_gene[7])) and bool(torch.isnan(r.r2_per_gene[7]))
        keep = torch.ones(D, dtype=torch.bool, device="cuda")
        keep[7] = False
        # r2 = 1 - sse / null: a relative error of 1e-5 in sse is an absolute one of 1e-5 sse / null in r2 (the bound of
        # tests/test_hip_gaussian_models.py::test_score_agrees_with_torch_in_fp64)
        for got, want in ((s.r2_per_gene[keep], r.r2_per_gene[keep]), (s.r2, r.r2)):
            assert bool(((got - want).abs() <= 1e-5 * (want.abs() + (1 - want).abs())).all())


def losses_of(loop, model, X, y, **kw):
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    torch.manual_seed(12)
    return loop(model, opt, X, y, steps=5, **kw)


def test_train_and_train_batched_follow_the_dense_run():
    from gpzoo.utilities import train, train_batched
    X, expr = problem()
    Xd, ed = X.cuda(), expr.cuda()
    yd = ed.to_dense()
    for loop, kw in ((train, {}), (train_batched, dict(batch_size=48))):
        sparse, dense = pair("WSVGP", X, expr)
        a = losses_of(loop, sparse, Xd, ed, **kw)
        b = losses_of(loop, dense, Xd, yd, **kw)
        print(loop.__name__, a, b)
        assert len(a) == len(b) == 5 and all(v == v for v in a + b)
        torch.testing.assert_close(torch.tensor(a), torch.tensor(b), rtol=1e-4, atol=0)
        assert bool((sparse.W < 0).any())
    with pytest.raises(TypeError, match="fused=True"):
        train(sparse, torch.optim.Adam(sparse.parameters()), Xd, ed, steps=1, fused=False)


def test_train_graphed_follows_the_eager_losses():
    """As tests/test_hip_gaussian_models.py::test_train_fused_and_graphed_agree: rtol 1e-4 over 10 steps."""
    from gpzoo.utilities import train
    X, expr = problem()
    Xd, ed = X.cuda(), expr.cuda()
    runs = {}
    for name, kw in (("fused", dict(fused=True)), ("graph", dict(fused=True, graph=True))):
        model = make("WSVGP", X, expr)
        opt = torch.optim.Adam(model.parameters(), lr=1e-2)
        torch.manual_seed(12)
        runs[name] = train(model, opt, Xd, ed, steps=10, E=3, **kw)
    print(runs)
    a, c = runs["fused"], runs["graph"]
    assert len(a) == len(c) == 10 and all(v == v for v in a + c)
    assert a[-1] < a[0]
    torch.testing.assert_close(torch.tensor(c), torch.tensor(a), rtol=1e-4, atol=0)


def test_forward_refuses_a_sparse_expression():
    X, expr = problem()
    model = make("WSVGP", X, expr)
    ed = expr.cuda()
    pY = model(X.cuda(), E=2)[0]
    with pytest.raises(TypeError, match="to_dense"):
        pY.log_prob(ed)
    assert pY.log_prob(ed.to_dense()).shape == (2, D, N)
