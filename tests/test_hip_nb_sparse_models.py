"""GPU: the count models with ``likelihood="nb"`` on a ``SparseCounts`` -- ``expected_loglik`` on the sparse counts and on
their batch view against the same call on ``to_dense()`` (same parameters, same eps), value and every parameter's gradient
within the step's tolerances (nb_cases.check: value rel 5e-5 / abs 1e-3, gradients rtol 1e-3 with atol 1e-3 max |dense|);
the mini-batch loop, the graphed loop and GraphedStep.check() on sparse counts.
Two spatial factors, two non-spatial ones where the model has them; N = 300 spots, D = 40 genes, M = 30 inducing points."""
import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

N, D, M, L, T, E, B = 300, 40, 30, 2, 2, 3, 77
KINDS = ("NSF2", "NSF", "Hybrid_NSF", "PNMF")


def problem(seed=41, theta=2.0, density=0.15):
    """Positions and thinned gamma-Poisson counts."""
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    X = (torch.rand(N, 2, generator=g) - 0.5) * 20
    rate = 0.5 + 4.0 * rng.random((D, 1)) * (0.3 + rng.random((1, N)))
    y = torch.from_numpy(rng.poisson(rng.gamma(theta, rate / theta)).astype(np.float32))
    y = y * (torch.rand(D, N, generator=g) < density)
    y[:, 17] = 0.0                      # a spot and a gene without counts
    y[5] = 0.0
    return X, y


def make(kind, X, y, seed=4):
    import gpzoo.gp as G
    import gpzoo.kernels as K
    import gpzoo.likelihoods as li
    torch.manual_seed(seed)
    kw = dict(likelihood="nb", theta0=10.0)
    if kind == "PNMF":
        prior = G.GaussianPrior(y, L=L)
        prior.mean = nn.Parameter(0.1 * torch.randn(L, N))
        prior.scale = nn.Parameter(0.1 + 0.3 * torch.rand(L, N))
        model = li.PNMF(prior, y, L=L, **kw)
    else:
        gp = G.WSVGP(K.NSF_RBF(sigma=1.0, lengthscale=4.0, L=L), dim=2, M=M, jitter=1e-2)
        gp.Z = nn.Parameter(X[:M].clone(), requires_grad=False)
        gp.mu = nn.Parameter(0.1 * torch.randn(L, M))
        gp.Lu = nn.Parameter(0.05 * torch.randn(L, M, M) - 0.5 * torch.eye(M))
        if kind == "Hybrid_NSF":
            model = li.Hybrid_NSF(gp, y, L=L, non_spatial_factors=T, **kw)
            model.mF = nn.Parameter(0.1 * torch.randn(T, N))
        else:
            model = getattr(li, kind)(gp, y, L=L, **kw)
    with torch.no_grad():               # distinct dispersions per gene, so a gradient landing on the wrong gene shows
        model.theta.copy_(torch.linspace(0.5, 6.0, D))
        model.V.copy_(0.5 + torch.rand(N))
    return model.cuda()


def value_and_grads(kind, X, y, counts, idx, eps):
    model = make(kind, X, y)
    ll = model.expected_loglik(X.cuda(), counts, idx=idx, E=E, eps=eps)[0]
    ll.backward()
    return float(ll), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("kind", KINDS)
def test_expected_loglik_takes_sparse_counts(kind):
    from gpzoo_amd.likelihoods import SparseCounts
    X, y = problem()
    sparse = SparseCounts(y).cuda()
    Lt = L + T if kind == "Hybrid_NSF" else L
    g = torch.Generator().manual_seed(8)
    idx = torch.randperm(N, generator=g)[:B].cuda()
    for tag, ix, n in (("all spots", None, N), ("batch view", idx, B)):
        eps = torch.randn(E, Lt, n, generator=g).cuda()
        counts = sparse if ix is None else sparse[:, ix]
        ls, gs = value_and_grads(kind, X, y, counts, ix, eps)
        ld, gd = value_and_grads(kind, X, y, counts.to_dense(), ix, eps)
        print(kind, tag, "dense", ld, "sparse", ls)
        assert ls == pytest.approx(ld, rel=5e-5, abs=1e-3)
        assert set(gs) == set(gd) and {"theta", "W", "V"} <= {k.split(".")[-1] for k in gd}
        for k in gd:
            sc = float(gd[k].abs().max()) + 1e-30
            print(f"  {k}: max err {float((gs[k] - gd[k]).abs().max()):.3e} of max |grad| {sc:.3e}")
            torch.testing.assert_close(gs[k], gd[k], rtol=1e-3, atol=1e-3 * sc, msg=lambda m: f"{kind} {tag} {k}: {m}")


def test_forward_still_refuses_sparse_counts():
    from gpzoo_amd.likelihoods import SparseCounts
    X, y = problem()
    model = make("NSF2", X, y)
    pY = model(X=X.cuda(), E=2)[0]
    with pytest.raises((TypeError, AttributeError, ValueError)):
        pY.log_prob(SparseCounts(y).cuda())


@pytest.mark.parametrize("kind", ["NSF2", "NSF"])
def test_train_batched_follows_the_dense_run(kind):
    """Three steps of train_batched(fused=True) from equal seeds: the losses of the dense run within the value's
    tolerance (rel 5e-5 / abs 1e-3)."""
    from gpzoo.utilities import train_batched
    from gpzoo_amd.likelihoods import SparseCounts
    X, y = problem()
    runs = []
    for counts in (y.cuda(), SparseCounts(y).cuda()):
        model = make(kind, X, y)
        opt = torch.optim.Adam(model.parameters(), lr=1e-2)
        torch.manual_seed(9)
        runs.append(train_batched(model, opt, X.cuda(), counts, steps=3, E=E, batch_size=128, fused=True))
    dense, sparse = runs
    print(kind, "dense", dense, "sparse", sparse)
    assert len(sparse) == len(dense) == 3
    for a, b in zip(sparse, dense):
        assert a == pytest.approx(b, rel=5e-5, abs=1e-3)


def test_graphed_loop_on_sparse_counts():
    """train(graph=True) captures the step with the sparse NB call in it and replays it; every replayed loss comes through
    GraphedStep.check() (sync_losses=True).  The graphed loop follows the eager fused one to 1e-4 relative, the bound of
    tests/test_hip_nb_models.py for the dense NB model, and the dense graphed run likewise."""
    from gpzoo.utilities import train
    from gpzoo_amd.likelihoods import SparseCounts
    X, y = problem()
    sparse = SparseCounts(y).cuda()
    runs = {}
    for name, counts, kw in (("eager", sparse, {}), ("graph", sparse, dict(graph=True)), ("graph_dense", y.cuda(), dict(graph=True))):
        model = make("NSF", X, y)
        opt = torch.optim.Adam(model.parameters(), lr=1e-2)
        torch.manual_seed(12)
        runs[name] = train(model, opt, X.cuda(), counts, steps=8, E=E, fused=True, **kw)
    print(runs)
    assert all(len(v) == 8 and all(u == u and abs(u) < float("inf") for u in v) for v in runs.values())
    torch.testing.assert_close(torch.tensor(runs["graph"]), torch.tensor(runs["eager"]), rtol=1e-4, atol=0)
    torch.testing.assert_close(torch.tensor(runs["graph"]), torch.tensor(runs["graph_dense"]), rtol=1e-4, atol=0)
