"""GPU: the sparse Poisson step (gpz_poisson_nsf_sparse, csrc/poisson_sparse.hip) against fp64 torch autograd of the DENSE
formula on the same counts (tests/sparse_poisson_cases.py; tests/test_sparse_poisson_cases.py checks the cases, the probes
and the sparse formulas on the CPU), and SparseCounts through the models and the training loops.

Bounds: the project's own for this operation, poisson_cases.LL_REL / LL_ABS / G_RTOL / G_ATOL,

  ll          pytest.approx(ref, rel=5e-5, abs=1e-3)
  gradients   assert_close(rtol=1e-3, atol=1e-3 max|ref|)

not loosened for this path.  Probe counts at the first and last entry of every gene chunk and at the first and last gene
and spot are worth at least ten tolerances in each output they feed (asserted on the CPU), so one dropped or doubled
non-zero fails.  Every comparison prints err / tolerance per output before it asserts; with GPZ_TEST_RECORD_DIR set the
figures are appended to poisson_sparse.jsonl there."""
import pytest
import torch
import torch.nn as nn

import poisson_cases as PC
import sparse_poisson_cases as SC
from helpers import record

pytestmark = pytest.mark.gpu


def _params(c):
    return [c[k].float().cuda() for k in ("mean", "scale", "eps", "W", "V")]


def counts_of(c):
    """The case's SparseCounts on the GPU (the batch view for a batch case)."""
    from gpzoo_amd.likelihoods import SparseCounts
    s = SparseCounts(c["y"].float()).cuda()
    return s[:, c["idx"].cuda()] if "idx" in c else s


def run(c, with_lgamma, counts=None):
    from gpzoo_amd import ops
    out = ops.poisson_nsf_sparse(*_params(c), counts_of(c) if counts is None else counts, None, with_lgamma)
    assert out[0].dtype == torch.float64 and all(t.dtype == torch.float32 for t in out[1:])
    return out


def figures(ref, got):
    fig = {"ll": abs(float(got[0]) - ref["ll"]) / float(PC.tolerance(ref, "ll"))}
    for nm, t in zip(PC.OUTPUTS, got[1:]):
        assert t.shape == ref[nm].shape and bool(torch.isfinite(t).all()), nm
        fig[nm] = float(((t.double().cpu() - ref[nm]).abs() / PC.tolerance(ref, nm)).max())
    return fig


def check(c, got, with_lgamma, tag, ref=None):
    ref = SC.reference(c, with_lgamma) if ref is None else ref
    fig = figures(ref, got)
    print(tag, "with_lgamma" if with_lgamma else "no_lgamma", "err/tol", {k: f"{v:.3g}" for k, v in fig.items()})
    record("poisson_sparse.jsonl", dict(case=str(tag), with_lgamma=with_lgamma, err_over_tol=fig), append=True)
    assert float(got[0]) == pytest.approx(ref["ll"], rel=PC.LL_REL, abs=PC.LL_ABS), tag
    for nm, t in zip(PC.OUTPUTS, got[1:]):
        torch.testing.assert_close(t.double().cpu(), ref[nm], rtol=PC.G_RTOL, atol=PC.G_ATOL * float(ref[nm].abs().max()),
                                   msg=lambda m: f"{nm} {tag}: {m}")


def _id(shape):
    return "N{}-D{}-Lt{}-E{}".format(*shape)


# --- 1. factor counts and samples ------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SC.FACTOR_SHAPES + SC.SAMPLE_SHAPES, ids=_id)
def test_factor_counts_and_samples(shape):
    """Lt at both ends of a kernel instance and at the largest; E = 33 crosses the sample group of the spot pass."""
    c = SC.shape_case(shape)
    with_lgamma = bool((shape[2] + shape[3]) % 2)
    check(c, run(c, with_lgamma), with_lgamma, shape)


# --- 2. chunk boundaries ---------------------------------------------------------------------------------------------

def test_gene_chunk_boundaries():
    """Gene rows of C - 1, C, C + 1, 2C + 1 and N = 1037 non-zeros (C from the plan query), probes at the first and last
    entry of every chunk; with and without the lgamma term, which the gradients do not depend on, bit for bit."""
    c = SC.chunk_case()
    counts = counts_of(c)
    plain, full = run(c, False, counts), run(c, True, counts)
    check(c, plain, False, "chunks")
    check(c, full, True, "chunks")
    for nm, a, b in zip(PC.OUTPUTS, plain[1:], full[1:]):
        assert torch.equal(a, b), nm


def test_fully_dense_spot_column():
    c = SC.dense_column_case()
    check(c, run(c, True), True, "dense_column")


# --- 3. degenerate structure -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["empties", "nnz1", "1x1", "values"])
@pytest.mark.parametrize("with_lgamma", [False, True])
def test_degenerate_structure(name, with_lgamma):
    """Empty rows and columns (the first and last among them), one non-zero, D = N = 1, counts >= 256 and non-integer."""
    c = dict(SC.all_cases())[name]
    check(c, run(c, with_lgamma), with_lgamma, name)


def test_no_counts_at_all():
    """nnz = 0: ll = -sum(rate) / E and the gradients are the dense terms alone."""
    c = SC.no_counts_case()
    got = run(c, True)
    check(c, got, True, "nnz0")
    rate = c["V"] * torch.matmul(c["W"], torch.exp(c["mean"] + c["scale"] * c["eps"]))
    assert float(got[0]) == pytest.approx(-float(rate.sum()) / c["E"], rel=PC.LL_REL, abs=PC.LL_ABS)
    assert bool((got[3] < 0).all()) and bool((got[4] < 0).all())


# --- 4. batches ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SC.BATCH_NAMES)
def test_batches(name):
    """y[:, idx] of an N = 1037 data set with an unsorted idx against the oracle on dense[:, idx]; the same spots through a
    SparseCounts built from dense[:, idx] agree within the same tolerance."""
    from gpzoo_amd.likelihoods import SparseCounts
    c = SC.batch_case(name)
    got = run(c, True)
    check(c, got, True, "batch_" + name)
    direct = run(c, True, SparseCounts(SC.batch_dense(c).float().cuda()))
    check(c, direct, True, "batch_" + name + "_direct")
    ref = SC.reference(c, True)
    assert float(got[0]) == pytest.approx(float(direct[0]), rel=PC.LL_REL, abs=PC.LL_ABS)
    for nm, a, b in zip(PC.OUTPUTS, got[1:], direct[1:]):
        torch.testing.assert_close(a, b, rtol=PC.G_RTOL, atol=PC.G_ATOL * float(ref[nm].abs().max()), msg=lambda m: f"{nm}: {m}")


# --- 5. agreement with the dense kernel ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["chunks", "values", "batch_B70"])
def test_agrees_with_the_dense_kernel(name):
    from gpzoo_amd import ops
    c = dict(SC.all_cases())[name]
    counts = counts_of(c)
    sparse = run(c, True, counts)
    dense = ops.poisson_nsf(*_params(c), counts.to_dense(), True)
    assert torch.equal(counts.to_dense().cpu().double(), SC.batch_dense(c))
    ref = SC.reference(c, True)
    fig = figures(dict(ref, ll=float(dense[0]), **{nm: t.double().cpu() for nm, t in zip(PC.OUTPUTS, dense[1:])}), sparse)
    print(name, "sparse vs dense kernel, err/tol", {k: f"{v:.3g}" for k, v in fig.items()})
    assert float(sparse[0]) == pytest.approx(float(dense[0]), rel=PC.LL_REL, abs=PC.LL_ABS)
    for nm, a, b in zip(PC.OUTPUTS, sparse[1:], dense[1:]):
        torch.testing.assert_close(a, b, rtol=PC.G_RTOL, atol=PC.G_ATOL * float(ref[nm].abs().max()), msg=lambda m: f"{nm}: {m}")


# --- 6. reproducibility ----------------------------------------------------------------------------------------------

def test_bitwise_reproducible_across_workspace_reuse():
    c, other = SC.chunk_case(), SC.batch_case("B70")
    counts, counts_other = counts_of(c), counts_of(other)
    first = run(c, True, counts)
    second = run(c, True, counts)
    run(other, True, counts_other)                     # another problem writes the same workspace
    third = run(c, True, counts)
    for a, b, d in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, d)


# --- 7. through the modules ------------------------------------------------------------------------------------------

def _problem():
    g = torch.Generator().manual_seed(31)
    N, D = 300, 60
    X = (torch.rand(N, 2, generator=g) - 0.5) * 10
    y = torch.poisson(3.0 * torch.rand(D, N, generator=g), generator=g) * (torch.rand(D, N, generator=g) < 0.08)
    return X, y


def _model(kind, y, X):
    from gpzoo.gp import SVGP, GaussianPrior
    from gpzoo.kernels import NSF_RBF
    from gpzoo.likelihoods import NSF2, Hybrid_NSF2
    g = torch.Generator().manual_seed(32)
    L, M = 3, 40
    gp = SVGP(NSF_RBF(L=L, lengthscale=2.0), dim=2, M=M, jitter=1e-2)
    gp.Z = nn.Parameter(X[:M].clone(), requires_grad=False)
    gp.mu = nn.Parameter(0.1 * torch.randn(L, M, generator=g))
    gp.Lu = nn.Parameter(0.05 * torch.randn(L, M, M, generator=g))
    if kind == "nsf2":
        model = NSF2(gp, y, L=L)
        model.W = nn.Parameter(torch.rand(y.shape[0], L, generator=g))
    else:
        prior = GaussianPrior(y, L=2)
        prior.mean = nn.Parameter(0.1 * torch.randn(2, y.shape[1], generator=g))
        prior.scale = nn.Parameter(0.3 * torch.rand(2, y.shape[1], generator=g))
        model = Hybrid_NSF2(gp, prior, y, L=L, T=2)
        model.sf.W = nn.Parameter(torch.rand(y.shape[0], L, generator=g))
        model.cf.W = nn.Parameter(torch.rand(y.shape[0], 2, generator=g))
    return model.cuda()


@pytest.mark.parametrize("kind", ["nsf2", "hybrid_nsf2"])
def test_expected_loglik_takes_sparse_counts(kind):
    """Value and .grad of every parameter: SparseCounts(y) against the dense-y call (same eps by the same seed)."""
    from gpzoo_amd.likelihoods import SparseCounts
    X, y = _problem()
    Xd, yd = X.cuda(), y.cuda()
    results = []
    for counts in (yd, SparseCounts(y).cuda()):
        model = _model(kind, counts, X)
        torch.manual_seed(5)
        ll = model.expected_loglik(Xd, counts, E=4)[0]
        ll.backward()
        results.append((float(ll), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
    (ld, gd), (ls, gs) = results
    print(kind, "ll dense", ld, "sparse", ls)
    assert ls == pytest.approx(ld, rel=PC.LL_REL, abs=PC.LL_ABS)
    assert set(gd) == set(gs) and len(gd) >= 4
    for n in gd:
        torch.testing.assert_close(gs[n], gd[n], rtol=PC.G_RTOL, atol=PC.G_ATOL * float(gd[n].abs().max()), msg=lambda m: f"{n}: {m}")


@pytest.mark.parametrize("loop,steps", [("train_batched", 3), ("train_graph", 3), ("train_graph", 5)])
def test_training_loops_take_sparse_counts(loop, steps):
    """Three steps of train_batched and of train(graph=True) on a SparseCounts: finite losses of the same shape, equal
    (rtol 1e-4) to the same loop on dense y with the same seeds.  (Three steps of the graphed loop are its eager warm-up
    and the capture; five also replay the captured step twice.)"""
    from gpzoo.utilities import train, train_batched
    from gpzoo_amd.likelihoods import SparseCounts
    X, y = _problem()
    Xd = X.cuda()
    runs = []
    for counts in (y.cuda(), SparseCounts(y).cuda()):
        model = _model("nsf2", counts, X)
        opt = torch.optim.Adam(model.parameters(), lr=1e-2)
        torch.manual_seed(9)
        if loop == "train_batched":
            runs.append(train_batched(model, opt, Xd, counts, steps=steps, E=3, batch_size=128))
        else:
            runs.append(train(model, opt, Xd, counts, steps=steps, E=3, graph=True))
    dense, sparse = runs
    print(loop, "dense", dense, "sparse", sparse)
    assert len(sparse) == len(dense) == steps and all(v == v and abs(v) < float("inf") for v in sparse)
    torch.testing.assert_close(torch.tensor(sparse), torch.tensor(dense), rtol=1e-4, atol=0)
