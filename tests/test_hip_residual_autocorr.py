"""GPU: the residual entries of gpzoo_amd/csrc/residual.hip against tests/residual_cases.py -- every residual element against
the fp64 oracle at the tolerance recorded there, gene lists, slabs, the sparse entry bit for bit against the dense one, the
Moran stage against the fp64 double sum of the entry's own residuals within the dense kernel's 1e-10, I end to end, the
planted structure, reproducibility on stale and poisoned memory, and the public path through the models."""
import functools

import numpy as np
import pytest
import torch
from torch import nn

import residual_cases as R

pytestmark = pytest.mark.gpu

MORAN_ATOL = 1e-10          # the bound tests/test_hip_gene_rank.py uses for the dense Moran kernel
CASES = tuple(r[0] for r in R.TABLE)
COMBOS = tuple((k, f) for k in R.KINDS for f in R.FAMILIES)


def _t(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype).cuda()


@functools.lru_cache(maxsize=None)
def _dev(name):
    c = R.make_case(name)
    return {k: _t(c[k]) for k in ("mean", "scale", "W", "V", "y", "theta")}


def _args(d, family, y=None):
    """(positional arguments, theta) of the ops entries for a case on the device."""
    return (d["mean"], d["scale"], d["W"], d["V"], d["y"] if y is None else y), (d["theta"] if family == "nb" else None)


def _residuals(d, kind, family, genes=None, y=None):
    from gpzoo_amd import ops
    a, th = _args(d, family, y)
    out = ops.count_residuals(*a, theta_pos=th, genes=genes, kind=kind)
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous()
    return out


def _moran(d, kind, family, nbr, y=None, **kw):
    from gpzoo_amd import ops
    a, th = _args(d, family, y)
    r = ops.residual_morans_i(*a, nbr, theta_pos=th, kind=kind, **kw)
    assert set(r) == {"I", "residual_mean", "residual_var"} and all(t.dtype == torch.float64 and t.is_cuda for t in r.values())
    return r


def _close(got, want, what):
    """1e-10 absolutely for values up to 1 in size (every I), relative to the value above: the variance of a gene that holds
    a probe count of thousands is of order 1e5, where 1e-10 absolute is the last bit of an fp64 number."""
    got, want = np.asarray(got), np.asarray(want)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(what, "max |got - want| / max(1, |want|)", err.max())
    assert got.shape == want.shape and np.isfinite(got).all() and err.max() <= MORAN_ATOL, what


# --- 1. the residual slab, element by element -------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_every_residual_matches_the_oracle(name):
    """|got - ref| <= RTOL |ref| + ATOL at every element, both kinds and both families; the probes (a count of thousands and a
    zero beside a large rate at the edges of tiles, waves and blocks) are elements like any other, so a misplaced or dropped
    element cannot hide."""
    c, d = R.make_case(name), _dev(name)
    for kind, family in COMBOS:
        got = _residuals(d, kind, family)
        assert got.shape == (c["B"], c["D"])
        fig = R.residual_figure(R.oracle_residuals(c, kind, family), got.T.double().cpu().numpy())
        print(name, kind, family, "max err / tol", fig)
        assert fig <= 1.0
    ref = R.oracle_residuals(c, "pearson", "poisson")
    for g, s, cnt in c["probes"]:
        assert (ref[g, s] > 100.0) if cnt > 0 else (ref[g, s] < -1.0), (g, s, cnt)


def test_gene_lists_repeat_skip_and_reorder():
    d, D = _dev("two_blocks"), 130
    lists = ([129, 0, 64, 64, 63, 0], list(range(0, D, 3)), list(range(D - 1, -1, -1)), [77],
             list(range(D)) + list(range(70)))                # more columns than genes
    for kind, family in COMBOS:
        full = _residuals(d, kind, family)
        for genes in lists:
            for g in (genes, torch.tensor(genes), torch.tensor(genes, dtype=torch.int32).cuda()):
                got = _residuals(d, kind, family, genes=g)
                assert got.shape == (130, len(genes)) and torch.equal(got, full[:, genes])


# --- 2. slabs ---------------------------------------------------------------------------------------------------------

def test_three_slabs_give_what_one_slab_gives():
    """D = 130 with slab_genes = 64 (three slabs, the last holding two genes) against slab_genes = 192 (one slab).  The
    residuals of a gene do not depend on its slab -- its mean and variance below come from the very same residuals -- but a
    slab of two columns is summed by other thread slots than one of 130, so the statistics agree to 1e-10, not bit for
    bit; the residual bits themselves are held by ``count_residuals`` in the Moran-stage test, which runs three slabs."""
    from gpzoo_amd import ops
    d = _dev("two_blocks")
    nbr = _t(R.case_table(R.make_case("two_blocks")), torch.int64)
    assert ops.residual_autocorr_plan(130, 130, 8, 0, 64)["n_slabs"] == 3
    assert ops.residual_autocorr_plan(130, 130, 8, 0, 192)["n_slabs"] == 1
    for kind, family in COMBOS:
        three, one = _moran(d, kind, family, nbr, slab_genes=64), _moran(d, kind, family, nbr, slab_genes=192)
        auto = _moran(d, kind, family, nbr)
        for k in three:
            _close(three[k].cpu().numpy(), one[k].cpu().numpy(), f"{kind} {family} {k}")
            assert torch.equal(auto[k], one[k])          # the plan's choice here is one slab of 192


# --- 3. sparse against dense ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sparse_case(which):
    """(device tensors with the edited y, SparseCounts on the device)."""
    from gpzoo.likelihoods import SparseCounts
    rng = np.random.default_rng(5)
    if which == "rows":                                        # rows of 511, 512 and 513 stored entries, B = 600
        c = R._draw("rows", 6, 600, 5, 0)
        y = c["y"] * (rng.random(c["y"].shape) < 0.05)
        for g, n in ((1, 511), (2, 512), (3, 513)):
            y[g] = 0.0
            y[g, rng.permutation(600)[:n]] = 1.0 + rng.poisson(3.0, n)
        y[0, 599] = 7.0                                        # the last spot, the first gene
    else:                                                      # a gene without stored entries, a gene stored at every spot
        c = dict(R.make_case("two_blocks"))
        y = c["y"] * (rng.random(c["y"].shape) < 0.3)
        y[17] = 0.0
        y[64] = np.maximum(c["y"][64], 1.0)
        y[129, 129] = 5000.0
    c = dict(c, y=y)
    d = {k: _t(c[k]) for k in ("mean", "scale", "W", "V", "y", "theta")}
    sc = SparseCounts(d["y"])
    lens = torch.diff(sc.row_ptr).cpu().tolist()
    if which == "rows":
        assert lens[1:4] == [511, 512, 513]
    else:
        assert lens[17] == 0 and lens[64] == 130
    return d, sc


@pytest.mark.parametrize("which", ["holes", "rows"])
def test_the_sparse_entry_gives_the_dense_entry_bits(which):
    """Every element: the zero-count fill and the stored entries' overwrite against the dense pass on the densified counts.
    SparseCounts drops explicit zeros, so there are none to store."""
    d, sc = _sparse_case(which)
    assert torch.equal(sc.to_dense(), d["y"])
    B = d["y"].shape[1]
    nbr = _t(R.random_table(B, 6, seed=3), torch.int64)
    genes = [3, 1, 1, 2, 0]
    for kind, family in COMBOS:
        dense = _residuals(d, kind, family)
        assert torch.equal(_residuals(d, kind, family, y=sc), dense)
        assert torch.equal(_residuals(d, kind, family, y=sc, genes=genes), dense[:, genes])
        a, b = _moran(d, kind, family, nbr, y=sc, slab_genes=64), _moran(d, kind, family, nbr, slab_genes=64)
        assert all(torch.equal(a[k], b[k]) for k in a)


# --- 4. the Moran stage -----------------------------------------------------------------------------------------------

def _check_moran_stage(d, nbr_np, slab_genes, what):
    nbr = _t(nbr_np, torch.int64)
    for kind, family in COMBOS:
        res = _residuals(d, kind, family).T.double().cpu().numpy()
        I, mean, var = R.morans_i(res, nbr_np)
        got = _moran(d, kind, family, nbr, slab_genes=slab_genes)
        _close(got["I"].cpu().numpy(), I, f"{what} {kind} {family} I")
        _close(got["residual_mean"].cpu().numpy(), mean, f"{what} {kind} {family} mean")
        _close(got["residual_var"].cpu().numpy(), var, f"{what} {kind} {family} var")


@pytest.mark.parametrize("K", [1, 6, 32])
def test_moran_stage_against_the_double_sum_of_its_own_residuals(K):
    """I, residual_mean and residual_var against the fp64 numpy Moran's I of the entry's own ``count_residuals`` output, to
    1e-10: a random table whose neighbours lie anywhere (other tiles; other spot slices and row chunks at B = 600), three
    slabs at D = 130."""
    _check_moran_stage(_dev("two_blocks"), R.random_table(130, K, seed=K), 64, f"two_blocks K={K}")
    d, _ = _sparse_case("rows")
    _check_moran_stage(d, R.random_table(600, K, seed=K), 0, f"rows K={K}")


def test_moran_stage_over_the_knn_table_of_random_points():
    from gpzoo_amd import ops
    X = np.random.default_rng(11).random((257, 2))
    nbr = ops.spatial_knn(_t(X, torch.float64), 6).cpu().numpy()
    np.testing.assert_array_equal(nbr, R.knn_table(X, 6))
    _check_moran_stage(_dev("lt20"), nbr, 64, "lt20 knn")


@pytest.mark.parametrize("bad", ["self", "beyond", "negative", "huge"])
def test_a_bad_table_raises_and_reads_nothing_out_of_range(bad):
    d = _dev("two_blocks")
    good = _t(R.random_table(130, 6, seed=1), torch.int64)
    nbr = good.clone()
    nbr[100, 3] = {"self": 100, "beyond": 130, "negative": -1, "huge": 1 << 40}[bad]
    with pytest.raises(ValueError, match=r"outside \[0, B\) or naming its own row"):
        _moran(d, "pearson", "nb", nbr)
    first = _moran(d, "pearson", "nb", good)                 # the clean table still gives the clean answer afterwards
    res = _residuals(d, "pearson", "nb").T.double().cpu().numpy()
    _close(first["I"].cpu().numpy(), R.morans_i(res, good.cpu().numpy())[0], "after a bad table")


# --- 5. end to end, planted structure ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_morans_i_end_to_end_against_the_oracle(name):
    c, d = R.make_case(name), _dev(name)
    nbr = R.case_table(c)
    for kind, family in COMBOS:
        want = R.morans_i(R.oracle_residuals(c, kind, family), nbr)[0]
        got = _moran(d, kind, family, _t(nbr, torch.int64))["I"].cpu().numpy()
        err = np.abs(got - want).max()
        print(name, kind, family, "max |I - oracle|", err, "of", R.I_ATOL)
        assert got.shape == (c["D"],) and err <= R.I_ATOL


def test_planted_structure_is_found():
    """No training: the model's rate is the null genes' true rate, four genes carry a pattern the rate does not contain."""
    from gpzoo.likelihoods import ResidualAutocorr, residual_autocorr
    from torch.distributions import Normal
    c = R.planted_case()
    d = {k: _t(c[k]) for k in ("mean", "scale", "W", "V", "y", "theta")}
    nbr = _t(c["nbr"], torch.int64)
    for kind, family in COMBOS:
        r = residual_autocorr([Normal(d["mean"], d["scale"])], [d["W"]], d["V"], d["y"], nbr,
                              theta_pos=d["theta"] if family == "nb" else None, kind=kind)
        assert isinstance(r, ResidualAutocorr) and all(t.dtype == torch.float64 for t in r)
        assert r.I.shape == r.z.shape == r.residual_mean.shape == r.residual_var.shape == (40,) and r.expected.dim() == 0
        z = r.z.cpu().numpy()
        print(kind, family, "planted z", z[c["planted"]], "largest null |z|", np.abs(z[~c["planted"]]).max())
        assert R.planted_conditions(z, c["planted"]) == (True, True, True)
        want = R.moran_z(R.morans_i(R.oracle_residuals(c, kind, family), c["nbr"])[0], c["nbr"])
        assert np.abs(z - want).max() <= R.I_ATOL / float(r.variance) ** 0.5          # I's tolerance, in units of z
    assert float(r.expected) == pytest.approx(-1.0 / 399.0)


# --- 6. reproducibility -----------------------------------------------------------------------------------------------

def _bits(t):
    t = t.cpu().numpy()
    return t.view(np.int64 if t.dtype == np.float64 else np.int32).copy()


def test_the_same_bits_on_a_second_call_and_on_poisoned_and_stale_memory():
    from gpzoo_amd import ops
    d, sc = _sparse_case("holes")
    nbr = _t(R.random_table(130, 6, seed=2), torch.int64)
    other = _dev("long_rows")
    other_nbr = _t(R.random_table(257, 3, seed=2), torch.int64)

    def run():
        out = []
        for y in (None, sc):
            out.append(_bits(_residuals(d, "deviance", "nb", y=y)))
            out += [_bits(t) for t in _moran(d, "deviance", "nb", nbr, y=y, slab_genes=64).values()]
        return out

    def poison_outputs():
        """Blocks of the outputs' sizes, filled with 0xFF and handed back to the allocator the entries draw from."""
        junk = [torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda") for n in (130 * 130 * 4, 130 * 8, 130 * 8, 130 * 8, 4)]
        del junk
    first = run()
    again = run()
    ws = ops._workspace(torch.device("cuda", torch.cuda.current_device()), 1)
    ws.fill_(0xFF)
    assert ws.numel() >= ops.residual_autocorr_plan(130, 130, 8, sc.nnz, 64)["partials_bytes"]
    poisoned = run()
    _moran(other, "pearson", "poisson", other_nbr)            # the leftovers of a call at another shape
    _residuals(other, "pearson", "poisson")
    stale = run()
    poison_outputs()
    fresh = run()
    for name, rerun in (("again", again), ("poisoned", poisoned), ("stale", stale), ("outputs", fresh)):
        for a, b in zip(first, rerun):
            np.testing.assert_array_equal(a, b, err_msg=name)


# --- 7. the public path -----------------------------------------------------------------------------------------------

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


def _same(a, b):
    return type(a) is type(b) and all(torch.equal(x, z) for x, z in zip(a, b))


@pytest.mark.parametrize("likelihood", ["poisson", "nb"])
def test_nsf_methods_equal_the_hand_assembled_call(likelihood):
    from gpzoo.likelihoods import NSF, ResidualAutocorr, residual_autocorr
    from gpzoo_amd import ops
    sp = torch.nn.functional.softplus
    g, X, y = _model_data()
    model = NSF(_gp(g, X), y.cpu(), L=L_M, likelihood=likelihood)
    model.W = nn.Parameter(torch.rand(D_M, L_M, generator=g))
    model.V = nn.Parameter(0.5 * torch.randn(N_M, generator=g))
    if likelihood == "nb":
        model.theta = nn.Parameter(2.0 * torch.randn(D_M, generator=g))
    model = model.cuda()
    theta = sp(model.theta.detach()) if likelihood == "nb" else None
    idx = torch.tensor([5, 129, 0, 77, 31, 64, 63, 100, 12, 90, 41], device="cuda")
    Vb = 0.5 + torch.rand(idx.numel(), generator=g).cuda()
    for kw, Xb, yb, Vp in ((dict(), X, y, None), (dict(idx=idx), X[idx], y[:, idx], None), (dict(idx=idx, V=Vb), X[idx], y[:, idx], Vb)):
        for kind in R.KINDS:
            r = model.residual_autocorr(X, yb, kind=kind, **kw)
            assert isinstance(r, ResidualAutocorr) and all(t.dtype == torch.float64 and not t.requires_grad for t in r)
            with torch.no_grad():
                qF = model.gp(X=Xb)[0]
                Vh = Vp if Vp is not None else (sp(model.V) if not kw else sp(model.V)[idx])
                hand = residual_autocorr([qF], [sp(model.W)], Vh, yb, ops.spatial_knn(Xb, 6), theta_pos=theta, kind=kind)
            assert _same(r, hand)
            assert _same(r, model.residual_autocorr(X, yb, kind=kind, graph=ops.spatial_knn(Xb, 6), **kw))
            genes = [7, 0, 79, 7]
            rows = model.residuals(X, yb, genes, kind=kind, **kw)
            full = ops.count_residuals(qF.mean, qF.scale, sp(model.W), Vh, yb, theta_pos=theta, kind=kind)
            assert rows.shape == (4, Xb.shape[0]) and torch.equal(rows, full.T[genes])
    assert all(p.grad is None for p in model.parameters())
    # the family: the model's own by default; a Poisson fit under a chosen theta; theta= refused for the Poisson family
    if likelihood == "poisson":
        assert _same(model.residual_autocorr(X, y), model.residual_autocorr(X, y, family="poisson"))
        assert not torch.equal(model.residual_autocorr(X, y, family="nb", theta=5.0).I, model.residual_autocorr(X, y).I)
    else:
        assert _same(model.residual_autocorr(X, y), model.residual_autocorr(X, y, family="nb"))
        assert not torch.equal(model.residual_autocorr(X, y, family="poisson").I, model.residual_autocorr(X, y).I)


def test_a_hybrid_with_idx_and_its_refusal_of_other_spots():
    from gpzoo.likelihoods import Hybrid_NSF, residual_autocorr
    from gpzoo_amd import ops
    from torch.distributions import Normal
    sp = torch.nn.functional.softplus
    g, X, y = _model_data()
    model = Hybrid_NSF(_gp(g, X), y.cpu(), L=L_M, non_spatial_factors=2, likelihood="nb")
    model.W = nn.Parameter(torch.rand(D_M, L_M, generator=g))
    model.W2 = nn.Parameter(torch.rand(D_M, 2, generator=g))
    model.mF = nn.Parameter(0.1 * torch.randn(2, N_M, generator=g))
    model.V = nn.Parameter(0.5 * torch.randn(N_M, generator=g))
    model = model.cuda()
    idx = torch.tensor([5, 129, 0, 77, 31, 64, 63, 100, 12, 90, 41], device="cuda")
    Vb = 0.5 + torch.rand(idx.numel(), generator=g).cuda()
    r = model.residual_autocorr(X, y[:, idx], idx=idx, V=Vb, kind="deviance")
    with torch.no_grad():
        qF = model.gp(X=X[idx])[0]
        qF2 = Normal(model.mF[:, idx], sp(model.scale_qF[:, idx]))
        hand = residual_autocorr([qF, qF2], [model.W, model.W2], Vb, y[:, idx], ops.spatial_knn(X[idx], 6),
                                 theta_pos=sp(model.theta), kind="deviance")
    assert _same(r, hand) and r.I.shape == (D_M,)
    rows = model.residuals(X, y[:, idx], [3, 1], idx=idx, V=Vb, kind="deviance")
    assert rows.shape == (2, idx.numel())
    with pytest.raises(ValueError, match="fitted spots"):
        model.residual_autocorr(X[:50], y[:, :50], V=torch.ones(50).cuda())
    with pytest.raises(ValueError, match="fitted spots"):
        model.deviance(X[:50], y[:, :50], V=torch.ones(50).cuda())
