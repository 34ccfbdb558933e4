"""GPU: the gene-wise dispersion fit of gpzoo_amd/csrc/gene_dispersion.hip against the fp64 oracle of tests/dispersion_cases.py
on every (N, sizes) case -- the status of every gene, the root through the oracle's score and in log theta, the gain and the
Poisson log-likelihood within 1e-11 of their scales, the boundary outputs exactly, bitwise reproducibility on stale and
poisoned scratch memory, the refusal of values that are no counts -- and the public path: gene_dispersion, rank_genes and a
count model started from the fit."""
import functools
import math

import numpy as np
import pytest
import torch

import dispersion_cases as DC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _counts(N, sizes):
    from gpzoo.likelihoods import SparseCounts
    return SparseCounts(torch.tensor(DC.case_counts(N, sizes))).cuda()


@functools.lru_cache(maxsize=None)
def _size(N, sizes):
    return torch.tensor(DC.case_sizes(N, sizes)).cuda()


@functools.lru_cache(maxsize=None)
def _fit(N, sizes, theta_range=DC.THETA_RANGE, max_iter=50):
    from gpzoo_amd import ops
    out = ops.gene_dispersion_sparse(_counts(N, sizes), _size(N, sizes), *theta_range, max_iter)
    theta, gain, pl, status, iterations = out
    assert all(t.dtype == torch.float64 and t.shape == (DC.D,) and t.is_cuda for t in (theta, gain, pl))
    assert all(t.dtype == torch.int32 and t.shape == (DC.D,) and t.is_cuda for t in (status, iterations))
    return tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("N,sizes", DC.CASES)
def test_fit_of_every_gene_matches_the_oracle(N, sizes):
    tol_t = DC.plan()["tol_t"]
    theta, gain, pl, status, iterations = _fit(N, sizes)
    o = DC.solve(N, sizes)
    np.testing.assert_array_equal(status, o["status"])
    assert (iterations <= 50).all() and (iterations[np.isin(status, (1, 2, 4))] == 0).all() and (iterations[status == 0] >= 1).all()
    genes = DC.genes(N, sizes)
    inner = np.nonzero(status == 0)[0]
    assert inner.size >= 20
    worst = dict(S=0.0, t=0.0)
    for d in inner:
        S, A, H = genes[d].score(theta[d])
        assert abs(S) <= DC.RTOL * A + abs(H) * tol_t, (d, S, A, H)
        bound = tol_t + DC.RTOL * o["A"][d] / abs(o["H"][d])
        assert abs(math.log(theta[d]) - math.log(o["theta"][d])) <= bound, (d, theta[d], o["theta"][d])
        worst["S"] = max(worst["S"], abs(S) / (DC.RTOL * A + abs(H) * tol_t))
        worst["t"] = max(worst["t"], abs(math.log(theta[d]) - math.log(o["theta"][d])) / bound)
    at = np.isin(status, (0, 2))
    gerr = np.abs(gain - o["gain"])[at] / o["gain_scale"][at]
    has = status != 4
    perr = np.abs(pl - o["poisson_loglik"])[has] / o["pl_scale"][has]
    print(N, sizes, "iterations mean", iterations[inner].mean(), "max", iterations.max(), "fraction of the bounds: S", worst["S"],
          "log theta", worst["t"], "gain err / scale", gerr.max(), "poisson_loglik err / scale", perr.max())
    assert (gerr <= DC.RTOL).all() and (perr <= DC.RTOL).all()
    # the boundary outputs, exactly
    lim = status == 1
    assert np.isposinf(theta[lim]).all() and (gain[lim] == 0.0).all() and not np.signbit(gain[lim]).any()
    assert (theta[status == 2] == DC.THETA_RANGE[0]).all()
    none = status == 4
    assert none[DC.row_kinds(N)["empty"]] and np.isnan(theta[none]).all() and (gain[none] == 0.0).all() and (pl[none] == 0.0).all()


@pytest.mark.parametrize("N,sizes", DC.NARROW_CASES)
def test_a_narrow_range_ends_at_its_bounds_where_the_oracle_says_so(N, sizes):
    theta, gain, pl, status, iterations = _fit(N, sizes, DC.NARROW_RANGE)
    o = DC.solve(N, sizes, DC.NARROW_RANGE)
    np.testing.assert_array_equal(status, o["status"])
    assert {0, 1, 2} <= set(status.tolist())
    assert np.isposinf(theta[status == 1]).all() and (gain[status == 1] == 0.0).all() and (theta[status == 2] == 1.0).all()
    inner = status == 0
    assert ((theta[inner] > 1.0) & (theta[inner] < 10.0)).all()
    at = np.isin(status, (0, 2))
    assert (np.abs(gain - o["gain"])[at] <= DC.RTOL * o["gain_scale"][at]).all()


@pytest.mark.parametrize("N,sizes", [(257, "ones"), (1037, "uniform")])
def test_no_iterations_return_the_moment_start(N, sizes):
    """max_iter = 0: every interior gene comes back at theta_0 = sum mu^2 / (sum (y - mu)^2 - sum y) clipped into the range,
    with status 3.  The kernel forms the denominator from sum y^2 - 2 p sum y size + p^2 sum size^2 - sum y: it carries
    1e-12 of those terms' sizes (fp64 sums of <= 4099 terms), so log theta_0 agrees within 1e-12 scale / |den|."""
    theta, gain, pl, status, iterations = _fit(N, sizes, DC.THETA_RANGE, 0)
    o = DC.solve(N, sizes)
    want = np.where(o["status"] == 0, 3, o["status"])
    np.testing.assert_array_equal(status, want)
    assert (iterations == 0).all()
    for d in np.nonzero(status == 3)[0]:
        g = DC.genes(N, sizes)[d]
        th0, den, scale = g.moment_start(DC.THETA_RANGE)
        if th0 in DC.THETA_RANGE:
            assert theta[d] == th0
        else:
            assert abs(math.log(theta[d]) - math.log(th0)) <= 1e-12 * scale / abs(den) + 1e-14, (d, theta[d], th0)
        want_gain, gscale = g.gain(theta[d])
        assert abs(gain[d] - want_gain) <= DC.RTOL * gscale
    some = _fit(N, sizes, DC.THETA_RANGE, 3)
    assert (some[4] <= 3).all() and (some[3][some[4] == 3] == 3).any()


def _bits(t):
    return t.cpu().numpy().view(np.int64 if t.dtype == torch.float64 else np.int32).copy()


def _poison(dev):
    from gpzoo_amd import ops
    ws = ops._workspace(dev, 1)
    ws.fill_(0xFF)
    return ws.numel()


@pytest.mark.parametrize("N,sizes", [(7, "holes"), (257, "ones"), (1037, "uniform"), (4099, "totals")])
def test_the_same_bits_on_poisoned_and_stale_scratch(N, sizes):
    from gpzoo_amd import ops
    c, size = _counts(N, sizes), _size(N, sizes)
    other_N = 257 if N != 257 else 1037

    def run():
        return [_bits(t) for t in ops.gene_dispersion_sparse(c, size)]
    first = run()
    again = run()
    assert _poison(c.device) >= ops.gene_dispersion_plan(N, DC.D, c.nnz)["partials_bytes"]
    poisoned = run()
    ops.gene_dispersion_sparse(_counts(other_N, "uniform"), _size(other_N, "uniform"))     # leftovers of another shape, unequal sizes
    ops.gene_deviance_sparse(_counts(other_N, "uniform"), _size(other_N, "uniform"), 0)
    stale = run()
    for name, rerun in (("again", again), ("poisoned", poisoned), ("stale", stale)):
        for a, b in zip(first, rerun):
            np.testing.assert_array_equal(a, b, err_msg=name)


@pytest.mark.parametrize("bad", [2.5, -1.0])
def test_a_value_that_is_no_count_raises_and_is_not_used(bad):
    from gpzoo.likelihoods import SparseCounts
    from gpzoo.utilities import gene_dispersion
    from gpzoo_amd import ops
    N, sizes = 257, "uniform"
    Y = DC.case_counts(N, sizes).copy()
    d = DC.row_kinds(N)["gp-2-1"]
    spot = int(np.nonzero(Y[d])[0][0])
    Y[d, spot] = bad
    c = SparseCounts(torch.tensor(Y)).cuda()
    with pytest.raises(ValueError, match="negative, not an integer"):
        ops.gene_dispersion_sparse(c, _size(N, sizes))
    with pytest.raises(ValueError, match="negative, not an integer"):
        gene_dispersion(c, _size(N, sizes))
    # not used: past the raise, the gene is fitted as if the entry were not stored (the other genes are untouched)
    import ctypes as C
    from gpzoo_amd import _lib
    lib = _lib.load()
    out = [torch.empty(DC.D, dtype=torch.float64).cuda() for _ in range(3)] + [torch.empty(DC.D, dtype=torch.int32).cuda() for _ in range(2)]
    info = torch.zeros(1, dtype=torch.int32).cuda()
    ws = torch.empty(4096, dtype=torch.uint8).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.gpz_gene_dispersion_sparse(p(c.row_ptr), p(c.row_spot), p(c.row_perm), p(c.col_val), p(_size(N, sizes)), N, DC.D, c.nnz,
                                        *DC.THETA_RANGE, 50, *(p(t) for t in out), p(info), p(ws), ws.numel(),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and int(info.item()) == 1
    theta, gain, pl, status, iterations = (t.cpu().numpy() for t in out)
    for got, want in zip((theta, gain, pl, status), _fit(N, sizes)):          # the other genes: the bits of the clean data set
        np.testing.assert_array_equal(np.delete(got, d).view(np.int64 if got.dtype == np.float64 else np.int32),
                                      np.delete(want, d).view(np.int64 if got.dtype == np.float64 else np.int32))
    Y[d, spot] = 0                                                            # gene d: the oracle's fit of the row without the entry
    g = DC.Gene(Y[d], DC.case_sizes(N, sizes))                                # (the entry's thread no longer adds it: not the same bits)
    S, A, H = g.score(theta[d])
    assert status[d] == 0 and abs(S) <= DC.RTOL * A + abs(H) * DC.plan()["tol_t"]
    want_gain, gscale = g.gain(theta[d])
    want_pl, pscale = g.poisson_loglik()
    assert abs(gain[d] - want_gain) <= DC.RTOL * gscale and abs(pl[d] - want_pl) <= DC.RTOL * pscale


def test_a_stored_count_at_a_spot_of_size_zero_raises():
    from gpzoo_amd import ops
    N = 257
    size = _size(N, "uniform").clone()
    size[5] = 0.0
    with pytest.raises(ValueError, match="size must be"):
        ops.gene_dispersion_sparse(_counts(N, "uniform"), size)
    size[5] = -1.0
    with pytest.raises(ValueError, match="size must be"):
        ops.gene_dispersion_sparse(_counts(N, "uniform"), size)


def test_gene_dispersion_and_rank_genes_through_the_public_names():
    from gpzoo.utilities import GeneDispersion, _rank_order, gene_dispersion, rank_genes
    N = 1037
    c = _counts(N, "holes")
    got = gene_dispersion(c)
    assert isinstance(got, GeneDispersion) and all(t.shape == (DC.D,) and t.device == c.device for t in got)
    theta, gain, pl, status, iterations = _fit(N, "holes")                     # size_factors=None: the spots' totals
    np.testing.assert_array_equal(_bits(got.theta), theta.view(np.int64))
    np.testing.assert_array_equal(_bits(got.poisson_loglik), pl.view(np.int64))
    np.testing.assert_array_equal(got.status.cpu().numpy(), status)
    np.testing.assert_array_equal(got.iterations.cpu().numpy(), iterations)
    g = torch.tensor(gain)
    assert torch.equal(got.lr.cpu(), 2.0 * g) and torch.equal(got.loglik.cpu(), torch.tensor(pl) + g)
    want_p = 0.5 * torch.erfc(torch.sqrt(g))
    want_p[torch.tensor(status == 1)] = 1.0
    want_p[torch.tensor(status == 4)] = float("nan")
    torch.testing.assert_close(got.pvalue.cpu(), want_p, rtol=1e-12, atol=0, equal_nan=True)
    assert bool((got.pvalue[got.status == 1] == 1).all()) and float(got.pvalue[DC.row_kinds(N)["spike"]]) < 1e-10
    sf = DC.case_sizes(N, "uniform")
    a = gene_dispersion(_counts(N, "uniform"), sf.reshape(-1, 1).copy(), theta_range=DC.NARROW_RANGE, max_iter=50)
    np.testing.assert_array_equal(_bits(a.theta), _fit(N, "uniform", DC.NARROW_RANGE)[0].view(np.int64))
    order, score = rank_genes(c, by="overdispersion")
    assert order.tolist() == _rank_order(got.lr).tolist() and torch.equal(score, got.lr[order])
    top, _ = rank_genes(c, by="overdispersion", nfeat=5)
    assert top.tolist() == order[:5].tolist()


def test_an_nsf_started_from_the_fit_takes_a_step():
    import gpzoo.gp as gp
    import gpzoo.kernels as k
    from gpzoo.likelihoods import NSF
    from gpzoo.utilities import gene_dispersion
    N = 257
    c = _counts(N, "totals")
    disp = gene_dispersion(c)
    theta0 = disp.theta.nan_to_num(nan=10.0).clamp(1e-2, 1e3)
    assert theta0.shape == (DC.D,) and bool(torch.isfinite(theta0).all()) and len(set(theta0.tolist())) > 10
    torch.manual_seed(0)
    X = torch.rand(N, 2) * 4 - 2
    prior = gp.WSVGP(k.NSF_RBF(sigma=1.0, lengthscale=1.0, L=3), dim=2, M=20, jitter=1e-2)
    prior.Z = torch.nn.Parameter(X[:20].clone(), requires_grad=False)
    prior.mu = torch.nn.Parameter(0.1 * torch.randn(3, 20))
    prior.Lu = torch.nn.Parameter(0.05 * torch.randn(3, 20, 20) - 0.5 * torch.eye(20))
    model = NSF(prior, torch.tensor(DC.case_counts(N, "totals")), L=3, likelihood="nb", theta0=theta0)
    torch.testing.assert_close(torch.nn.functional.softplus(model.theta.detach()).double(), theta0.cpu(), rtol=1e-5,
                               atol=1.1e-5)                                      # init_softplus floors by 1e-5
    model = model.cuda()
    value = model.expected_loglik(X.cuda(), c, E=3)[0]
    assert value.dim() == 0 and bool(torch.isfinite(value))
    value.backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert model.theta.grad is not None and grads and all(bool(torch.isfinite(g).all()) for g in grads)
