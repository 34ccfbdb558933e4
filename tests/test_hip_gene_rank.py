"""GPU: the per-gene scores of gpzoo_amd/csrc/gene_rank.hip against the fp64 oracles of tests/gene_rank_cases.py -- Moran's I
of every gene (gpz_gene_morans_i_sparse) within the dense kernel's 1e-10, the gene deviance (gpz_gene_deviance_sparse) within
1e-11 of its own scale with exact sums and counts, both bitwise reproducible on stale and poisoned scratch memory -- and
the public path: gene_autocorr, rank_genes, select_genes and the NMF start on the selected genes."""
import functools

import numpy as np
import pytest
import torch

import gene_rank_cases as G

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _counts(N, variant):
    from gpzoo.likelihoods import SparseCounts
    return SparseCounts(torch.tensor(G.counts(N, variant))).cuda()


@functools.lru_cache(maxsize=None)
def _values(N, variant):
    """(SparseExpression on the device, its dense (D, N) fp32 array on the host): log_normalize(counts, center=False)."""
    e, dense = G.log_values(N, variant)
    return e.cuda(), dense


@functools.lru_cache(maxsize=None)
def _nbr(N, K):
    return torch.tensor(G.graph(N, K)).cuda()


def _inputs(N, variant):
    """(name, sparse object on the device, dense array on the host) for raw counts and log-normalised values."""
    e, dense = _values(N, variant)
    return (("counts", _counts(N, variant), G.counts(N, variant)), ("log", e, dense))


@pytest.mark.parametrize("N,K", G.GRAPHS)
def test_morans_i_of_every_gene_matches_the_oracle(N, K):
    """rtol = 0, atol = 1e-10 (the dense kernel's bound), NaN exactly where the oracle has it."""
    from gpzoo_amd import ops
    kinds = G.row_kinds(N)
    for variant in G.VARIANTS:
        for name, sparse, dense in _inputs(N, variant):
            got = ops.gene_morans_i_sparse(sparse, _nbr(N, K))
            assert got.dtype == torch.float64 and got.shape == (G.D,) and got.is_cuda
            got = got.cpu().numpy()
            want = G.moran_oracle(dense, G.graph(N, K))
            nan = np.isnan(want)
            assert nan[kinds["empty"]]
            np.testing.assert_array_equal(np.isnan(got), nan)
            print(N, K, variant, name, "max |I - oracle|", np.abs(got - want)[~nan].max())
            np.testing.assert_allclose(got[~nan], want[~nan], rtol=0, atol=G.MORAN_ATOL)


DEVIANCE_RUNS = (("poisson", "totals"), ("poisson", "factors"), ("binomial", "totals"))


@pytest.mark.parametrize("N", G.NS)
def test_gene_deviance_matches_the_oracle(N):
    """|got - want| <= 1e-11 scale_d per gene, scale_d = 2 (sum |saturated terms| + |null terms|); sums and counts exact."""
    from gpzoo_amd import ops
    for variant in G.VARIANTS:
        c = _counts(N, variant)
        for family, which in DEVIANCE_RUNS:
            size = G.sizes(N, variant, which)
            s, n, dev = ops.gene_deviance_sparse(c, torch.tensor(size).cuda(), 1 if family == "binomial" else 0)
            assert all(t.dtype == torch.float64 and t.shape == (G.D,) and t.is_cuda for t in (s, n, dev))
            o = G.deviance_oracle(G.counts(N, variant), size, family)
            np.testing.assert_array_equal(s.cpu().numpy(), o["sum"])
            np.testing.assert_array_equal(n.cpu().numpy(), o["count"])
            err = np.abs(dev.cpu().numpy() - o["deviance"])
            print(N, variant, family, which, "max |deviance - oracle| / scale", (err / np.maximum(o["scale"], 1e-300)).max())
            assert (err <= G.DEVIANCE_RTOL * o["scale"]).all(), np.nonzero(err > G.DEVIANCE_RTOL * o["scale"])[0]
            assert dev[G.row_kinds(N)["empty"]] == 0


def test_binomial_terms_with_y_equal_to_the_size_are_zero():
    """Every stored count is its spot's whole total (scry's na.rm=TRUE): the saturated sum is 0 and only the null is left;
    a single gene holding every count has p = 1 and deviance 0."""
    from gpzoo.likelihoods import SparseCounts
    from gpzoo.utilities import gene_deviance
    Y = np.array([[3.0, 0.0, 0.0, 1.0], [0.0, 2.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]], dtype=np.float32)
    got = gene_deviance(SparseCounts(torch.tensor(Y)).cuda(), "binomial").cpu().numpy()
    o = G.deviance_oracle(Y, Y.sum(axis=0), "binomial")
    assert (np.abs(got - o["deviance"]) <= G.DEVIANCE_RTOL * o["scale"]).all() and got[2] == 0 and (got[:2] > 0).all()
    one = gene_deviance(SparseCounts(torch.tensor(Y[:1])).cuda(), "binomial")
    assert one.tolist() == [0.0]


def _bits(t):
    return t.cpu().numpy().view(np.int64).copy()


def _poison(dev):
    from gpzoo_amd import ops
    ws = ops._workspace(dev, 1)
    ws.fill_(0xFF)
    return ws.numel()


@pytest.mark.parametrize("N,K", G.GRAPHS)
def test_both_entries_give_the_same_bits_on_poisoned_and_stale_scratch(N, K):
    from gpzoo_amd import ops
    c, (e, _) = _counts(N, "holes"), _values(N, "holes")
    size = torch.tensor(G.sizes(N, "holes", "totals")).cuda()
    other_N = 257 if N != 257 else 1037
    other = _counts(other_N, "full")

    def run():
        out = [_bits(ops.gene_morans_i_sparse(v, _nbr(N, K))) for v in (c, e)]
        out += [_bits(t) for fam in (0, 1) for t in ops.gene_deviance_sparse(c, size, fam)]
        return out
    first = run()
    again = run()
    assert _poison(c.device) >= ops.gene_rank_plan(N, G.D, c.nnz, K=K)["partials_bytes"]
    poisoned = run()
    ops.gene_morans_i_sparse(other, _nbr(other_N, 1))             # the leftovers of a call at another shape
    ops.gene_deviance_sparse(other, torch.tensor(G.sizes(other_N, "full", "factors")).cuda(), 0)
    stale = run()
    for name, rerun in (("again", again), ("poisoned", poisoned), ("stale", stale)):
        for a, b in zip(first, rerun):
            np.testing.assert_array_equal(a, b, err_msg=name)


@pytest.mark.parametrize("bad", ["self", "beyond", "negative", "huge"])
def test_a_corrupted_table_raises_as_morans_i_does(bad):
    from gpzoo_amd import ops
    N, K = 257, 6
    nbr = _nbr(N, K).clone()
    row = 200
    nbr[row, 3] = {"self": row, "beyond": N, "negative": -1, "huge": 1 << 40}[bad]
    dense = torch.tensor(G.counts(N, "full")).cuda()
    with pytest.raises(ValueError, match=r"outside \[0, N\) or naming its own row"):
        ops.morans_i(dense.T.contiguous(), nbr)
    with pytest.raises(ValueError, match=r"outside \[0, N\) or naming its own row"):
        ops.gene_morans_i_sparse(_counts(N, "full"), nbr)
    from gpzoo.utilities import gene_autocorr
    with pytest.raises(ValueError, match="naming its own row"):
        gene_autocorr(_counts(N, "full"), graph=nbr)
    # the clean table still gives the clean answer afterwards
    got = ops.gene_morans_i_sparse(_counts(N, "full"), _nbr(N, K)).cpu().numpy()
    want = G.moran_oracle(G.counts(N, "full"), G.graph(N, K))
    np.testing.assert_allclose(got, want, rtol=0, atol=G.MORAN_ATOL, equal_nan=True)


@pytest.mark.parametrize("N,K", [(7, 6), (257, 1), (1037, 6), (1037, 32)])
def test_gene_autocorr_over_a_given_graph(N, K):
    from gpzoo.likelihoods import SparseExpression
    from gpzoo.utilities import GeneAutocorr, gene_autocorr, log_normalize
    c = _counts(N, "holes")
    e = log_normalize(c)                                         # centred: the offset does not change I
    assert isinstance(e, SparseExpression) and float(e.offset.abs().max()) > 0
    nbr = _nbr(N, K)
    a, b = gene_autocorr(e, graph=nbr), gene_autocorr(e.values, graph=nbr)
    assert isinstance(a, GeneAutocorr) and all(t.dtype == torch.float64 and t.is_cuda for t in a)
    np.testing.assert_array_equal(_bits(a.I), _bits(b.I))
    dense = gene_autocorr(e.values.to_dense(), graph=nbr)
    nan = torch.isnan(a.I)
    assert torch.equal(nan, torch.isnan(dense.I)) and bool(nan.any()) and not bool(nan.all())
    np.testing.assert_allclose(a.I[~nan].cpu().numpy(), dense.I[~nan].cpu().numpy(), rtol=0, atol=G.MORAN_ATOL)
    EI, VI = G.moments_oracle(G.graph(N, K))
    for r in (a, dense):
        assert r.expected.shape == () and r.variance.shape == () and r.z.shape == (G.D,)
        assert abs(float(r.expected) - EI) <= 1e-12 * abs(EI)
        assert abs(float(r.variance) - VI) <= G.moments_bound(N, K, VI)
    if K < N - 1:
        want_z = (a.I.cpu().numpy() - EI) / np.sqrt(VI)
        np.testing.assert_allclose(a.z.cpu().numpy(), want_z, rtol=1e-10, atol=0, equal_nan=True)


def test_gene_autocorr_builds_the_graph_from_coords():
    from gpzoo_amd import ops
    from gpzoo.utilities import gene_autocorr
    N = 1037
    X = np.random.default_rng(5).random((N, 2)) * 10.0
    c = _counts(N, "full")
    got = gene_autocorr(c, X, n_neighs=6)
    nbr = ops.spatial_knn(torch.tensor(X).cuda(), 6)
    np.testing.assert_array_equal(_bits(got.I), _bits(ops.gene_morans_i_sparse(c, nbr)))
    want = G.moran_oracle(G.counts(N, "full"), nbr.cpu().numpy())
    np.testing.assert_allclose(got.I.cpu().numpy(), want, rtol=0, atol=G.MORAN_ATOL, equal_nan=True)
    EI, VI = G.moments_oracle(nbr.cpu().numpy())
    assert abs(float(got.variance) - VI) <= 1e-12 * VI and float(got.expected) == EI
    assert gene_autocorr(c, torch.tensor(X, dtype=torch.float32).cuda()).I.shape == (G.D,)      # n_neighs defaults to 6


def test_gene_deviance_through_the_public_name():
    from gpzoo.utilities import gene_deviance
    N = 1037
    c = _counts(N, "holes")
    Y = G.counts(N, "holes")
    sf = G.sizes(N, "holes", "factors")
    for got, o in ((gene_deviance(c), G.deviance_oracle(Y, G.sizes(N, "holes", "totals"), "poisson")),
                   (gene_deviance(c, "binomial"), G.deviance_oracle(Y, G.sizes(N, "holes", "totals"), "binomial")),
                   (gene_deviance(c, size_factors=sf.reshape(-1, 1)), G.deviance_oracle(Y, sf, "poisson")),
                   (gene_deviance(c, "poisson", torch.tensor(sf, dtype=torch.float32)),
                    G.deviance_oracle(Y, sf.astype(np.float32), "poisson"))):
        assert got.dtype == torch.float64 and got.shape == (G.D,) and got.device == c.device
        assert (np.abs(got.cpu().numpy() - o["deviance"]) <= G.DEVIANCE_RTOL * o["scale"]).all()


@pytest.mark.parametrize("by", ["deviance", "binomial_deviance", "moran"])
def test_rank_select_and_start_the_factorisation(by):
    from gpzoo.utilities import gene_autocorr, gene_deviance, log_normalize, rank_genes, regularized_nmf
    N = 1037
    c = _counts(N, "holes")
    kw = dict(graph=_nbr(N, 6)) if by == "moran" else {}
    order, score = rank_genes(c, by=by, **kw)
    assert order.dtype == torch.int64 and order.shape == (G.D,) and score.dtype == torch.float64 and order.device == c.device
    assert sorted(order.tolist()) == list(range(G.D))
    full = {"deviance": lambda: gene_deviance(c), "binomial_deviance": lambda: gene_deviance(c, "binomial"),
            "moran": lambda: gene_autocorr(log_normalize(c, center=False), graph=_nbr(N, 6)).I}[by]()
    np.testing.assert_array_equal(_bits(score), _bits(full[order]))
    want = np.argsort(-full.cpu().numpy(), kind="stable")        # decreasing, NaN last, ties in gene order
    assert order.tolist() == want.tolist()
    top, top_score = rank_genes(c, by=by, nfeat=12, **kw)
    assert top.tolist() == order[:12].tolist() and torch.equal(top_score, score[:12])
    sel = c.select_genes(top)
    assert tuple(sel.shape) == (12, N) and torch.equal(sel.to_dense(), c.to_dense()[top])
    F, W = regularized_nmf(sel.T, L=3, max_iter=5, solver="mu", beta_loss="kullback-leibler", init="nndsvdar", random_state=0)
    assert F.shape == (N, 3) and W.shape == (12, 3) and np.isfinite(F).all() and np.isfinite(W).all()


def test_select_genes_on_the_device_equals_the_dense_construction():
    from gpzoo.likelihoods import SparseCounts
    c = _counts(257, "full")
    genes = torch.tensor(np.random.default_rng(2).permutation(G.D)[:20]).cuda()
    got, want = c.select_genes(genes), SparseCounts(c.to_dense()[genes])
    for k in SparseCounts._PARTS:
        assert getattr(got, k).is_cuda and torch.equal(getattr(got, k), getattr(want, k)), k
    e = _values(257, "full")[0]
    sub = e.select_genes(genes.cpu().tolist())
    assert sub.device == e.device and torch.equal(sub.to_dense(), e.to_dense()[genes])


def test_views_and_wrong_types_are_refused_on_the_device_path():
    from gpzoo_amd import ops
    from gpzoo.utilities import gene_autocorr, gene_deviance, rank_genes
    N = 257
    c, (e, _) = _counts(N, "full"), _values(N, "full")
    idx = torch.arange(0, N, 2).cuda()
    size = torch.tensor(G.sizes(N, "full", "totals")).cuda()
    for bad in (c[:, idx], c.T, e, c.to_dense()):
        with pytest.raises(TypeError):
            ops.gene_deviance_sparse(bad, size, 0)
        with pytest.raises(TypeError):
            gene_deviance(bad)
        with pytest.raises(TypeError):
            rank_genes(bad)
    for bad in (c[:, idx], e[:, idx], c.T, c.to_dense()):
        with pytest.raises(TypeError):
            ops.gene_morans_i_sparse(bad, _nbr(N, 6))
    for bad in (c[:, idx], e[:, idx], c.T):
        with pytest.raises(TypeError):
            gene_autocorr(bad, graph=_nbr(N, 6))
    with pytest.raises(ValueError):
        ops.gene_deviance_sparse(c, size.float(), 0)
    with pytest.raises(ValueError):
        ops.gene_deviance_sparse(c, size[:-1], 0)
    with pytest.raises(ValueError):
        ops.gene_deviance_sparse(c, size, 2)
    with pytest.raises(ValueError):
        ops.gene_morans_i_sparse(c, _nbr(N, 6)[:-1])
    with pytest.raises(ValueError, match="K = 33"):
        ops.gene_morans_i_sparse(c, torch.zeros((N, 33), dtype=torch.int64).cuda())
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.gene_morans_i_sparse(c.cpu(), _nbr(N, 6))
