"""GPU: the NB deviance entries (gpz_nb_deviance, gpz_nb_deviance_sparse; csrc/nb_deviance.hip) against the fp64 oracle of
tests/nb_deviance_cases.py, and ``deviance(family=...)`` of the models.

The reference has no such function; the oracle is fp64 torch on the same fp32 inputs through
torch.distributions.NegativeBinomial and Poisson (tests/test_nb_deviance_cases.py checks it against the written-out
formulas, the cases, and the sharpness of every probe on the CPU).

Bounds: the project's Poisson ones (poisson_cases.LL_REL / LL_ABS / G_RTOL / G_ATOL),

  total, sum_y, sum_mu, null_total, loglik, poisson_loglik                    |got - ref| <= 5e-5 |ref| + 1e-3
  per_gene, per_spot, null_per_gene, loglik_per_gene, loglik_per_spot,
  poisson_loglik_per_gene                                                     |got - ref| <= 1e-3 |ref| + 1e-3 max|ref|

Tile and chunk boundaries come from the plan queries; none is restated.  Every comparison prints err / tolerance per
output before it asserts; with GPZ_TEST_RECORD_DIR set the figures are appended to nb_deviance.jsonl there."""
import pytest
import torch
import torch.nn as nn

import deviance_cases as DC
import nb_deviance_cases as NC
from helpers import record

pytestmark = pytest.mark.gpu

FLAGS = [True, False]


def dplan(N, D, Lt):
    from gpzoo_amd import ops
    return ops.nb_deviance_plan(N, D, Lt)


def gene_chunk():
    from gpzoo_amd import ops
    return ops.nb_deviance_sparse_plan(2000, 2000, 6, 5, 1000)["gene_chunk"]


def _params(c):
    return [c[k].float().cuda() for k in ("mean", "scale", "W", "V", "theta")]


def run_dense(c, flag=True):
    from gpzoo_amd import ops
    return ops.nb_deviance(*_params(c), c["y"].float().cuda(), flag)


def counts_of(c):
    from gpzoo_amd.likelihoods import SparseCounts
    return SparseCounts(c["y"].float()).cuda()


def run_sparse(c, flag=True, counts=None):
    from gpzoo_amd import ops
    return ops.nb_deviance_sparse(*_params(c), counts_of(c) if counts is None else counts, None, flag)


def check(c, got, flag, tag):
    ref = NC.oracle(c, flag)
    assert set(got) == set(NC.OUTPUTS)
    for k in NC.OUTPUTS:
        assert got[k].dtype == torch.float64 and not got[k].requires_grad, k
    fig = NC.figures(ref, got)
    print(tag, "lognormal" if flag else "plug-in", "err/tol", {k: f"{v:.3g}" for k, v in fig.items()})
    record("nb_deviance.jsonl", dict(case=str(tag), lognormal_mean=flag, err_over_tol=fig), append=True)
    for k, v in fig.items():
        assert v <= 1.0, (tag, k, v)


def bits_equal(a, b):
    return all(torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)) for k in NC.OUTPUTS)


def mid_positions():
    return DC.dense_positions(NC.MID[0], NC.MID[1], dplan(*NC.MID))


# --- 1. factor instances ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ["dense", "sparse"])
@pytest.mark.parametrize("Lt", DC.FACTOR_COUNTS)
def test_factor_instances(Lt, entry):
    c = NC.dense_case(130, 80, Lt, dplan(130, 80, Lt))
    for flag in FLAGS:
        check(c, run_dense(c, flag) if entry == "dense" else run_sparse(c, flag), flag, f"{entry}-Lt{Lt}")


# --- 2. tile edges ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("e", DC.EDGE_SPOTS, ids=lambda e: f"{e[0]}ts{e[1]:+d}")
def test_spot_tile_edges(e):
    """N one below, at and one above the plan's spots per tile, 1, two tiles + 1, and N no multiple of 4.  With N = 1, V = 1
    and counts in {0, 1} the null model reproduces the counts: its deviance must be exactly 0."""
    N = DC.edge(dplan(130, 80, 5)["spots_per_tile"], e)
    D = DC.ONE_SPOT_GENES if N == 1 else 37
    c = NC.dense_case(N, D, 5, dplan(N, D, 5))
    for flag in FLAGS:
        for tag, got in ((f"N{N}", run_dense(c, flag)), (f"sparse-N{N}", run_sparse(c, flag))):
            check(c, got, flag, tag)
            if N == 1:
                assert bool((got["null_per_gene"] == 0).all()) and float(got["null_total"]) == 0.0


@pytest.mark.parametrize("unit,e", [("genes_per_tile", e) for e in DC.EDGE_GENES] + [("genes_per_block", e) for e in DC.EDGE_BLOCKS],
                         ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]:+d}")
def test_gene_tile_and_block_edges(unit, e):
    """D one below, at and one above the plan's genes per tile and every workgroup block boundary."""
    D = DC.edge(dplan(130, 80, 5)[unit], e)
    c = NC.dense_case(70, D, 5, dplan(70, D, 5))
    assert dplan(70, D, 5)["gene_slices"] == -(-D // dplan(70, D, 5)["genes_per_block"])
    for flag in FLAGS:
        check(c, run_dense(c, flag), flag, f"D{D}")
        check(c, run_sparse(c, flag), flag, f"sparse-D{D}")


@pytest.mark.parametrize("theta", [None, NC.THETA_LARGE], ids=["spread", "large"])
def test_spot_slices(theta):
    """More than one spot slice: per-gene partial slabs added in slice order, probes on both sides of every slice cut; with
    one large theta the probes are sharp in the null deviance and the Poisson log density too."""
    p = dplan(*DC.SLICED)
    assert p["spot_slices"] > 1
    c = NC.dense_case(*DC.SLICED, p, theta=theta)
    for flag in FLAGS:
        check(c, run_dense(c, flag), flag, "sliced")
        check(c, run_sparse(c, flag), flag, "sparse-sliced")


def test_unaligned_counts_pointer():
    """y at an element offset that is no multiple of 16 bytes (a view): rows are then read element by element."""
    from gpzoo_amd import ops
    c = NC.dense_case(128, 37, 5, dplan(128, 37, 5))
    buf = torch.zeros(37 * 128 + 1, dtype=torch.float32, device="cuda")
    y = buf[1:].view(37, 128)
    y.copy_(c["y"].float())
    assert y.data_ptr() % 16 == 4
    check(c, ops.nb_deviance(*_params(c), y, True), True, "unaligned-y")


# --- 3. zeros --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ["dense", "sparse"])
def test_all_zero_counts(entry):
    """Every output is its zero part; the null deviance exactly 0, explained NaN."""
    from gpzoo_amd.likelihoods import NBDeviance, SparseCounts, nb_deviance
    c = NC.zeros_cases()["all_zero"]
    for flag in FLAGS:
        got = run_dense(c, flag) if entry == "dense" else run_sparse(c, flag)
        check(c, got, flag, f"{entry}-all-zero")
        assert float(got["sum_y"]) == 0.0 and float(got["null_total"]) == 0.0 and bool((got["null_per_gene"] == 0).all())
        assert float(got["total"]) == pytest.approx(-2.0 * float(got["loglik"]), rel=1e-6)
        assert float(got["poisson_loglik"]) == pytest.approx(-float(got["sum_mu"]), rel=1e-6)
    mean, scale, W, V, theta = _params(c)
    y = c["y"].float().cuda()
    r = nb_deviance([torch.distributions.Normal(mean, scale)], [W], V, theta, SparseCounts(y) if entry == "sparse" else y)
    assert isinstance(r, NBDeviance) and bool(torch.isnan(r.explained)) and bool(torch.isnan(r.explained_per_gene).all())
    assert float(r.mean) == pytest.approx(float(r.total) / (c["D"] * c["N"]), rel=1e-12)


@pytest.mark.parametrize("entry", ["dense", "sparse"])
def test_a_gene_and_a_spot_without_counts(entry):
    c = NC.zeros_cases()["empty_gene_and_spot"]
    for flag in FLAGS:
        got = run_dense(c, flag) if entry == "dense" else run_sparse(c, flag)
        check(c, got, flag, f"{entry}-empty-gene-and-spot")
        assert float(got["null_per_gene"][17]) == 0.0
        # exactly the zero part over the row / the column
        assert float(got["per_gene"][17]) == pytest.approx(-2.0 * float(got["loglik_per_gene"][17]), rel=1e-5)
        assert float(got["per_spot"][66]) == pytest.approx(-2.0 * float(got["loglik_per_spot"][66]), rel=1e-5)


# --- 4. sparse rows, views -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("theta", [None, NC.THETA_LARGE], ids=["spread", "large"])
def test_gene_chunk_boundaries(theta):
    """Gene rows of exactly one chunk, one chunk + 1 and three chunks of non-zeros (length from the plan), probes at the first
    and last entry of every chunk; against the oracle and against the dense entry."""
    c = NC.chunk_case(gene_chunk(), theta=theta)
    chunk = gene_chunk()
    assert (c["y"] != 0).sum(1).tolist()[1:4] == [chunk, chunk + 1, 3 * chunk]
    for flag in FLAGS:
        check(c, run_sparse(c, flag), flag, "chunks")
    check(c, run_dense(c), True, "chunks-dense")


def test_no_stored_values():
    c = NC.zeros_cases()["all_zero"]
    counts = counts_of(c)
    assert counts.nnz == 0
    check(c, run_sparse(c, True, counts), True, "nnz0")


def test_view_of_the_counts():
    """y[:, idx] with an unsorted idx of 37 of 130 spots that holds the first and last spot and leaves out a spot with a
    probe: the oracle on the dense columns, the dense entry on the same columns, per-spot outputs in idx's order."""
    from gpzoo_amd import ops
    c, idx = NC.view_case()
    v = NC.view(c, idx)
    counts = counts_of(c)
    sub = counts[:, idx.cuda()]
    for flag in FLAGS:
        got = ops.nb_deviance_sparse(*_params(v), sub, None, flag)
        check(v, got, flag, "view")
        same = ops.nb_deviance_sparse(*_params(v), counts, idx.cuda(), flag)           # idx= is shorthand for the view
        assert bits_equal(got, same)
        dense = ops.nb_deviance(*_params(v), counts.to_dense()[:, idx.cuda()], flag)
        check(v, dense, flag, "view-dense")
    assert got["per_spot"].shape == (37,) and got["loglik_per_spot"].shape == (37,)
    d, n = DC.VIEW_EXCLUDED_PROBE
    assert n not in idx.tolist() and (d, n) in {(a, b) for a, b, _ in c["probes"]}


# --- 5. dense against sparse, theta extremes, reproducibility --------------------------------------------------------

def test_dense_against_sparse_on_the_same_counts():
    c = NC.make_probe_case(*NC.MID, mid_positions(), seed=9, density=0.2)
    for flag in FLAGS:
        a, b = run_dense(c, flag), run_sparse(c, flag)
        check(c, a, flag, "same-dense")
        check(c, b, flag, "same-sparse")
        fig = NC.figures({k: a[k].cpu() for k in NC.OUTPUTS}, b)
        print("sparse against dense err/tol", fig)
        assert max(fig.values()) <= 1.0


@pytest.mark.parametrize("which", ["small", "large", "mixed"])
def test_theta_extremes(which):
    """theta = 0.05 and 1e6 for every gene, and the whole range 0.3 ... 1e6 within every 16-gene wave tile."""
    theta = dict(small=NC.THETA_SMALL, large=NC.THETA_LARGE,
                 mixed=NC.mixed_theta(NC.MID[1], dplan(*NC.MID)["genes_per_tile"]))[which]
    c = NC.make_probe_case(*NC.MID, mid_positions(), seed=dict(small=12, large=13, mixed=14)[which], theta=theta)
    for flag in FLAGS:
        check(c, run_dense(c, flag), flag, f"theta-{which}")
        check(c, run_sparse(c, flag), flag, f"sparse-theta-{which}")


def test_the_poisson_limit_against_the_poisson_entry():
    """theta = 1e7: the NB deviance, its null and per-gene / per-spot sums against ops.poisson_deviance run on the same
    inputs, and loglik against poisson_loglik, within the tolerances (tests/test_nb_deviance_cases.py: the fp64 difference
    is below a third of them)."""
    from gpzoo_amd import ops
    c = NC.limit_case()
    for flag in FLAGS:
        po = ops.poisson_deviance(*_params(c)[:4], c["y"].float().cuda(), flag)
        ref = {k: v.cpu() for k, v in po.items()}
        for tag, got in (("limit", run_dense(c, flag)), ("sparse-limit", run_sparse(c, flag))):
            check(c, got, flag, tag)
            fig = DC.figures(ref, got)
            print(tag, "against the Poisson entry err/tol", fig)
            assert max(fig.values()) <= 1.0
            fig = NC.figures({k: got["poisson_" + k].cpu() for k in ("loglik", "loglik_per_gene")},
                             dict(loglik=got["loglik"], loglik_per_gene=got["loglik_per_gene"]), ("loglik", "loglik_per_gene"))
            assert max(fig.values()) <= 1.0, fig


@pytest.mark.parametrize("entry", ["dense", "sparse"])
def test_two_calls_agree_bit_for_bit(entry):
    cases = [NC.dense_case(*DC.SLICED, dplan(*DC.SLICED))] if entry == "dense" else [NC.chunk_case(gene_chunk())]
    cases.append(NC.dense_case(130, 80, 20, dplan(130, 80, 20)))
    for c in cases:
        run = run_dense if entry == "dense" else run_sparse
        first = run(c)
        first = {k: first[k].clone() for k in NC.OUTPUTS}
        from gpzoo_amd import ops
        ops._workspace(torch.device("cuda", torch.cuda.current_device()), 1).fill_(0x5A)      # another workspace content
        assert bits_equal(first, run(c))


# --- 6. models -------------------------------------------------------------------------------------------------------

N_M, M_M, D_M, L_M = 130, 16, 80, 3


def _model_data():
    g = torch.Generator().manual_seed(73)
    X = 4.0 * torch.rand(N_M, 2, generator=g) - 2.0
    y = torch.poisson(2.0 * torch.rand(D_M, N_M, generator=g), generator=g)
    return g, X.cuda(), y.cuda()


def _gp(g, X):
    import gpzoo.gp as G
    import gpzoo.kernels as K
    gp = G.WSVGP(K.NSF_RBF(L=L_M, lengthscale=2.0), dim=2, M=M_M, jitter=1e-2)
    gp.Z = nn.Parameter(X.cpu()[:M_M].clone(), requires_grad=False)
    gp.mu = nn.Parameter(0.3 * torch.randn(L_M, M_M, generator=g))
    gp.Lu = nn.Parameter(0.05 * torch.randn(L_M, M_M, M_M, generator=g) - 0.5 * torch.eye(M_M))
    return gp


def _nsf(g, X, y, likelihood):
    from gpzoo.likelihoods import NSF
    model = NSF(_gp(g, X), y.cpu(), L=L_M, likelihood=likelihood)
    model.W = nn.Parameter(torch.rand(D_M, L_M, generator=g))
    model.V = nn.Parameter(0.5 * torch.randn(N_M, generator=g))
    if likelihood == "nb":
        model.theta = nn.Parameter(2.0 * torch.randn(D_M, generator=g))
    return model.cuda()


def _same(a, b):
    return type(a) is type(b) and all(torch.equal(x, z) or bool((torch.isnan(x) & torch.isnan(z)).all()) for x, z in zip(a, b))


def test_model_deviance_families():
    from gpzoo.likelihoods import NBDeviance, PoissonDeviance, nb_deviance
    sp = torch.nn.functional.softplus
    g, X, y = _model_data()
    model = _nsf(g, X, y, "nb")
    r = model.deviance(X, y, family="nb")
    assert isinstance(r, NBDeviance)
    assert all(isinstance(t, torch.Tensor) and t.dtype == torch.float64 and not t.requires_grad for t in r)
    assert all(p.grad is None for p in model.parameters())
    with torch.no_grad():
        qF = model.gp(X=X)[0]
        hand = nb_deviance([qF], [sp(model.W)], sp(model.V), sp(model.theta), y)
    assert _same(r, hand) and _same(r, model.deviance(X, y, family="model"))
    torch.testing.assert_close(r.theta, sp(model.theta).detach().float().double())
    # against the oracle on the model's own moments
    f = lambda t: t.detach().float().double().cpu()                                    # noqa: E731
    c = dict(mean=f(qF.mean), scale=f(qF.scale), W=f(sp(model.W)), V=f(sp(model.V)), y=f(y), theta=f(sp(model.theta)))
    got = {k: getattr(r, k) for k in NC.OUTPUTS}
    fig = NC.figures(NC.oracle(c), got)
    print("NSF nb err/tol", fig)
    assert max(fig.values()) <= 1.0
    # the Poisson deviance is what it was: the default call, bit for bit
    a, b = model.deviance(X, y), model.deviance(X, y, family="poisson")
    assert isinstance(a, PoissonDeviance) and _same(a, b)
    # a SparseCounts view goes through the sparse entry
    from gpzoo_amd.likelihoods import SparseCounts
    idx = torch.tensor([5, 129, 0, 77, 31, 64, 63], device="cuda")
    rb = model.deviance(X, SparseCounts(y)[:, idx], idx=idx, family="nb")
    rd = model.deviance(X, y[:, idx], idx=idx, family="nb")
    assert rb.per_spot.shape == (7,) and rb.loglik_per_spot.shape == (7,)
    fig = NC.figures({k: getattr(rd, k).cpu() for k in NC.OUTPUTS}, {k: getattr(rb, k) for k in NC.OUTPUTS})
    print("view: sparse against dense err/tol", fig)
    assert max(fig.values()) <= 1.0


def test_a_poisson_fitted_model_under_a_chosen_theta():
    from gpzoo.likelihoods import NBDeviance, PoissonDeviance
    g, X, y = _model_data()
    model = _nsf(g, X, y, "poisson")
    assert isinstance(model.deviance(X, y, family="model"), PoissonDeviance)
    with pytest.raises(ValueError, match="theta"):
        model.deviance(X, y, family="nb")
    r = model.deviance(X, y, family="nb", theta=10.0)
    assert isinstance(r, NBDeviance) and bool((r.theta == 10.0).all()) and r.theta.shape == (D_M,)
    per_gene = model.deviance(X, y, family="nb", theta=torch.full((D_M,), 10.0))
    assert _same(r, per_gene)
    # the same rate: the Poisson log density is that of the Poisson deviance's model, and the NB one differs from it
    p = model.deviance(X, y)
    assert float(r.sum_mu) == pytest.approx(float(p.sum_mu), rel=1e-6) and float(r.loglik) != float(r.poisson_loglik)


def test_a_hybrid_with_idx():
    import gpzoo.gp as G
    from gpzoo.likelihoods import Hybrid_NSF2, NBDeviance
    g, X, y = _model_data()
    prior = G.GaussianPrior(y.cpu(), L=2)
    prior.mean = nn.Parameter(0.1 * torch.randn(2, N_M, generator=g))
    prior.scale = nn.Parameter(0.1 + 0.3 * torch.rand(2, N_M, generator=g))
    model = Hybrid_NSF2(_gp(g, X), prior, y.cpu(), L=L_M, T=2, likelihood="nb")
    model.sf.W = nn.Parameter(torch.rand(D_M, L_M, generator=g))
    model.cf.W = nn.Parameter(torch.rand(D_M, 2, generator=g))
    model.V = nn.Parameter(0.5 * torch.randn(N_M, generator=g))
    model = model.cuda()
    idx = torch.tensor([5, 129, 0, 77, 31, 64, 63], device="cuda")
    r = model.deviance(X, y[:, idx], idx=idx, family="nb")
    assert isinstance(r, NBDeviance) and r.per_spot.shape == (7,) and r.per_gene.shape == (D_M,)
    sp = torch.nn.functional.softplus
    with torch.no_grad():
        q1, q2 = model.sf.prior(X=X[idx])[0], model.cf.prior.forward_batched(idx)[0]
    f = lambda t: t.detach().float().double().cpu()                                    # noqa: E731
    c = dict(mean=torch.cat([f(q1.mean), f(q2.mean)]), scale=torch.cat([f(q1.scale), f(q2.scale)]),
             W=torch.cat([f(sp(model.sf.W)), f(sp(model.cf.W))], dim=1), V=f(sp(model.V)[idx]), y=f(y[:, idx]),
             theta=f(sp(model.theta)))
    fig = NC.figures(NC.oracle(c), {k: getattr(r, k) for k in NC.OUTPUTS})
    print("Hybrid_NSF2 nb err/tol", fig)
    assert max(fig.values()) <= 1.0
