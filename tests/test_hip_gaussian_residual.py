"""GPU: the Gaussian residual entries (gpzoo_amd/csrc/residual_gaussian.h behind the driver of csrc/residual.hip) against
tests/gaussian_residual_cases.py -- every residual element against the fp64 oracle at the tolerance recorded there, gene
lists, the sparse entries bit for bit against the dense ones, the statistics stage against the fp64 double sums of the
entry's own residuals, I and C end to end, the permutation entries, reproducibility on stale and poisoned memory, the planted
structure through the permutation p-values, and the public path through RSF, FA and PNMF."""
import functools

import numpy as np
import pytest
import torch
from torch import nn

import gaussian_residual_cases as G
import geary_cases as Y

pytestmark = pytest.mark.gpu

STAGE_ATOL = 1e-10          # the bound the count tests use for the column passes
CASES = tuple(r[0] for r in G.TABLE)
STAT_FIELDS = ("I", "C", "residual_mean", "residual_var", "kurtosis")
PERM_FIELDS = ("value", "n_ge", "n_le", "sim_mean", "sim_m2", "sims")
PARTS = ("mean", "scale", "W", "b", "sd", "y")


def _t(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype).cuda()


def _on_device(c):
    return {k: _t(c[k]) for k in PARTS}


@functools.lru_cache(maxsize=None)
def _dev(name):
    return _on_device(G.make_case(name))


def _model(d):
    return d["mean"], d["scale"], d["W"], d["b"], d["sd"]


def _residuals(d, kind, genes=None, y=None):
    from gpzoo_amd import ops
    out = ops.gaussian_residuals(*_model(d), d["y"] if y is None else y, genes=genes, kind=kind)
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous()
    return out


def _stats(d, kind, nbr, y=None, **kw):
    from gpzoo_amd import ops
    r = ops.gaussian_residual_stats(*_model(d), d["y"] if y is None else y, nbr, kind=kind, **kw)
    assert tuple(r) == STAT_FIELDS and all(t.dtype == torch.float64 and t.is_cuda for t in r.values())
    return r


def _perm(d, kind, nbr, perms, stat, y=None, **kw):
    from gpzoo_amd import ops
    r, mom = ops.gaussian_residual_autocorr_perm(*_model(d), d["y"] if y is None else y, nbr, perms, kind=kind, stat=stat,
                                                 return_sims=True, **kw)
    assert r.stat == stat and r.n_ge.dtype == r.n_le.dtype == torch.int32 and tuple(mom) == STAT_FIELDS[2:]
    return r, mom


def _bits(t):
    t = t.cpu().numpy()
    return t.view(np.int64 if t.dtype == np.float64 else np.int32).copy()


def _all_bits(r, mom):
    return [_bits(getattr(r, f)) for f in PERM_FIELDS] + [_bits(t) for t in mom.values()]


def _close(got, want, what):
    """1e-10 absolutely for values up to 1 in size (every I and C), relative to the value above: the variance of a gene
    with sd = 1e-2 that holds a probe of hundreds is of order 1e7."""
    got, want = np.asarray(got), np.asarray(want)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(what, "max |got - want| / max(1, |want|)", err.max())
    assert got.shape == want.shape and np.isfinite(got).all() and err.max() <= STAGE_ATOL, what


# --- 1. the residual slab, element by element -------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_every_residual_matches_the_oracle(name):
    """|got - ref| <= RTOL |ref| + CTOL 2^-24 S / den at every element, all three kinds; the probes (a y of hundreds beside
    yhat of order 1 at the edges of tiles, waves and blocks) are elements like any other, so a misplaced or dropped element
    cannot hide."""
    c, d = G.make_case(name), _dev(name)
    for kind in G.KINDS:
        got = _residuals(d, kind)
        assert got.shape == (c["B"], c["D"])
        fig = G.residual_figure(c, kind, got.T.double().cpu().numpy())
        print(name, kind, "max err / tol", fig)
        assert fig <= 1.0
    ref = G.oracle_residuals(c, "response")
    for g, s, y in c["probes"]:
        assert abs(ref[g, s]) > 100.0 and np.sign(ref[g, s]) == np.sign(y), (g, s, y)


# --- 2. gene lists ----------------------------------------------------------------------------------------------------

def test_gene_lists_repeat_skip_and_reorder():
    d, D = _dev("two_blocks"), 130
    lists = ([129, 0, 64, 64, 63, 0], list(range(0, D, 3)), list(range(D - 1, -1, -1)), [77],
             list(range(D)) + list(range(70)))                # more columns than genes
    for kind in G.KINDS:
        full = _residuals(d, kind)
        for genes in lists:
            for g in (genes, torch.tensor(genes), torch.tensor(genes, dtype=torch.int32).cuda()):
                got = _residuals(d, kind, genes=g)
                assert got.shape == (130, len(genes)) and torch.equal(got, full[:, genes])


# --- 3. sparse against dense ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sparse_case(which, offset):
    """(device tensors with y = the dense array, the SparseExpression on the device)."""
    c, v, off = G.sparse_case(which, offset)
    return _on_device(c), G.sparse_expression(v, off, device="cuda")


@pytest.mark.parametrize("offset", G.OFFSETS)
@pytest.mark.parametrize("which", G.SPARSE_CASES)
def test_the_sparse_entries_give_the_dense_entries_bits(which, offset):
    """Every element: the fill at y = (float)(-offset) and the stored entries' overwrite against the dense pass on
    expr.to_dense(); then all five statistics at slab_genes = 64."""
    d, expr = _sparse_case(which, offset)
    assert torch.equal(expr.to_dense(), d["y"])
    B = d["y"].shape[1]
    nbr = _t(G.random_table(B, 6, seed=3), torch.int64)
    genes = [3, 1, 1, 2, 0]
    for kind in G.KINDS:
        dense = _residuals(d, kind)
        assert torch.equal(_residuals(d, kind, y=expr), dense)
        assert torch.equal(_residuals(d, kind, y=expr, genes=genes), dense[:, genes])
        a, b = _stats(d, kind, nbr, y=expr, slab_genes=64), _stats(d, kind, nbr, slab_genes=64)
        for f in STAT_FIELDS:
            np.testing.assert_array_equal(_bits(a[f]), _bits(b[f]), err_msg=f"{kind} {f}")


# --- 4. the statistics stage ------------------------------------------------------------------------------------------

def _check_stage(d, nbr_np, what):
    from gpzoo_amd import ops
    nbr = _t(nbr_np, torch.int64)
    for kind in G.KINDS:
        res = _residuals(d, kind)
        want = G.spatial_stats(res.T.double().cpu().numpy(), nbr_np)
        three, one = _stats(d, kind, nbr, slab_genes=64), _stats(d, kind, nbr, slab_genes=192)
        cols = ops.spatial_stats(res, nbr)
        for f, col in zip(STAT_FIELDS, (cols.I, cols.C, cols.mean, cols.var, cols.kurtosis)):
            _close(three[f].cpu().numpy(), want[f], f"{what} {kind} {f}")
            _close(three[f].cpu().numpy(), col.cpu().numpy(), f"{what} {kind} {f} against spatial_stats")
            _close(three[f].cpu().numpy(), one[f].cpu().numpy(), f"{what} {kind} {f} three slabs against one")


@pytest.mark.parametrize("K", [1, 6, 32])
def test_statistics_against_the_double_sums_of_the_own_residuals(K):
    """I, C, mean, variance and kurtosis against the fp64 numpy double sums of the entry's own ``gaussian_residuals`` output
    and against ``ops.spatial_stats`` on that output, to 1e-10: 130 genes in three slabs of 64 against one slab, at one
    256-row chunk (B = 130) and at two (B = 257); a random table whose neighbours lie anywhere."""
    from gpzoo_amd import ops
    assert ops.gaussian_residual_plan(130, 130, 8, K, 0, 0, 64)["n_slabs"] == 3
    assert ops.gaussian_residual_plan(257, 130, 20, K, 0, 0, 192)["n_slabs"] == 1
    _check_stage(_dev("two_blocks"), G.random_table(130, K, seed=K), f"two_blocks K={K}")
    _check_stage(_dev("lt20"), G.random_table(257, K, seed=K), f"lt20 K={K}")


# --- 5. end to end ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_i_and_c_end_to_end_against_the_oracle(name):
    c, d = G.make_case(name), _dev(name)
    nbr_np = G.case_table(c)
    nbr = _t(nbr_np, torch.int64)
    got = {}
    for kind in ("pearson", "predictive"):
        want = G.spatial_stats(G.oracle_residuals(c, kind), nbr_np)
        got[kind] = _stats(d, kind, nbr)
        ei = np.abs(got[kind]["I"].cpu().numpy() - want["I"]).max()
        ec = np.abs(got[kind]["C"].cpu().numpy() - want["C"]).max()
        print(name, kind, "max |I - oracle|", ei, "of", G.I_ATOL, "max |C - oracle|", ec, "of", G.C_ATOL)
        assert got[kind]["I"].shape == (c["D"],) and ei <= G.I_ATOL and ec <= G.C_ATOL
    gap = (got["pearson"]["I"] - _stats(d, "response", nbr)["I"]).abs().max().item()
    print(name, "max |I(pearson) - I(response)|", gap)
    assert gap <= G.I_ATOL


# --- 6. permutations --------------------------------------------------------------------------------------------------

def _some_perms(B, P, seed=0):
    rng = np.random.default_rng(900 + seed)
    return np.stack([np.arange(B)] + [rng.permutation(B) for _ in range(P - 1)]).astype(np.int32)      # the identity first


@pytest.mark.parametrize("name", ["two_blocks", "long_rows"])
def test_the_identity_the_batch_size_and_the_relabelled_table(name):
    """The identity row reproduces the observed I and C bit for bit; nothing depends on perm_batch; sims[:, p] is the stats
    entry on the table relabelled by permutation p, T[pi[i], m] = pi[nbr[i, m]], to 1e-10."""
    c, d = G.make_case(name), _dev(name)
    B = c["B"]
    nbr_np, perms_np = G.random_table(B, 6, seed=4), _some_perms(B, 19)
    nbr, perms = _t(nbr_np, torch.int64), _t(perms_np, torch.int32)
    for kind in ("pearson", "predictive"):
        observed = _stats(d, kind, nbr, slab_genes=64)
        for stat, f in (("moran", "I"), ("geary", "C")):
            r, mom = _perm(d, kind, nbr, perms, stat, slab_genes=64)
            np.testing.assert_array_equal(_bits(r.value), _bits(observed[f]))
            np.testing.assert_array_equal(_bits(r.sims[:, 0].contiguous()), _bits(observed[f]))
            for k in mom:
                np.testing.assert_array_equal(_bits(mom[k]), _bits(observed[k]))
            first = _all_bits(r, mom)
            for pb in (1, 3, 16):
                for a, b in zip(first, _all_bits(*_perm(d, kind, nbr, perms, stat, slab_genes=64, perm_batch=pb))):
                    np.testing.assert_array_equal(a, b, err_msg=f"perm_batch={pb}")
            assert (r.n_ge.cpu().numpy() + r.n_le.cpu().numpy() >= 19).all() and (r.n_ge >= 1).all() and (r.n_le >= 1).all()
            for p in (1, 7, 18):
                pi = perms_np[p].astype(np.int64)
                T = np.empty_like(nbr_np)
                T[pi] = pi[nbr_np]
                want = _stats(d, kind, _t(T, torch.int64), slab_genes=64)[f]
                _close(r.sims[:, p].cpu().numpy(), want.cpu().numpy(), f"{name} {kind} {stat} permutation {p}")


@pytest.mark.parametrize("table", sorted(Y.ENUM_TABLES))
def test_all_5040_relabellings_give_the_randomisation_moments(table):
    """mean_sim and var_sim of I and C over every relabelling of seven spots are the analytic randomisation moments at the
    device's own kurtosis, to 1e-12."""
    from gpzoo_amd.utilities import _autocorr_moments
    d = _dev("one_gene")
    nbr, perms = _t(Y.ENUM_TABLES[table], torch.int64), _t(Y.enum_perms(), torch.int32)
    for kind in ("pearson", "predictive"):
        for stat, E, V in (("moran", "EI", "VI"), ("geary", "EC", "VC")):
            r, mom = _perm(d, kind, nbr, perms, stat)
            m = _autocorr_moments(nbr, mom["kurtosis"])
            mean, var = r.sim_mean.cpu().numpy(), (r.sim_m2 / 5040).cpu().numpy()
            em, ev = np.abs(mean - float(m[E])).max(), np.abs(var - m[V + "_rand"].cpu().numpy()).max()
            print(table, kind, stat, "|mean - E|", em, "|var - V_rand|", ev)
            assert em <= 1e-12 and ev <= 1e-12


# --- 7. reproducibility -----------------------------------------------------------------------------------------------

def test_the_same_bits_on_a_second_call_and_on_poisoned_and_stale_memory():
    from gpzoo_amd import ops
    d, expr = _sparse_case("holes", "uncentred")
    nbr = _t(G.random_table(130, 6, seed=2), torch.int64)
    perms = _t(_some_perms(130, 5), torch.int32)
    other = _dev("long_rows")
    other_nbr = _t(G.random_table(257, 3, seed=2), torch.int64)

    def run():
        out = []
        for y in (None, expr):
            for kind in ("pearson", "predictive"):
                out.append(_bits(_residuals(d, kind, y=y)))
                out += [_bits(t) for t in _stats(d, kind, nbr, y=y, slab_genes=64).values()]
                out += _all_bits(*_perm(d, kind, nbr, perms, "geary", y=y, slab_genes=64, perm_batch=2))
        return out

    def poison_outputs():
        """Blocks of the outputs' sizes, filled with 0xFF and handed back to the allocator the entries draw from."""
        junk = [torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda") for n in (130 * 130 * 4, 130 * 8, 130 * 8, 130 * 8, 130 * 5 * 8, 4)]
        del junk
    first = run()
    again = run()
    ws = ops._workspace(torch.device("cuda", torch.cuda.current_device()), 1)
    ws.fill_(0xFF)                                               # every fp32 and fp64 of the scratch a NaN
    assert ws.numel() >= ops.gaussian_residual_plan(130, 130, 8, 6, 5, expr.nnz, 64, 2)["partials_bytes"]
    poisoned = run()
    _stats(other, "predictive", other_nbr)                      # the leftovers of a call at another shape
    _residuals(other, "pearson")
    stale = run()
    poison_outputs()
    fresh = run()
    for name, rerun in (("again", again), ("poisoned", poisoned), ("stale", stale), ("outputs", fresh)):
        for a, b in zip(first, rerun):
            np.testing.assert_array_equal(a, b, err_msg=name)


# --- 8. planted structure ---------------------------------------------------------------------------------------------

def test_planted_structure_has_the_smallest_p_values():
    """No training: the model is the null genes' true mean, ten of a hundred genes carry a smooth factor it does not contain."""
    from gpzoo.likelihoods import ResidualAutocorrPerm, ResidualGearyPerm, gaussian_residual_autocorr
    from torch.distributions import Normal
    c = G.planted_case()
    d = _on_device(c)
    nbr, perms = _t(c["nbr"], torch.int64), _t(c["perms"], torch.int32)
    qF = [Normal(d["mean"], d["scale"])]
    for kind in ("pearson", "predictive"):
        r = gaussian_residual_autocorr(qF, [d["W"]], d["b"], d["sd"], d["y"], nbr, kind=kind, perms=perms)
        g = gaussian_residual_autocorr(qF, [d["W"]], d["b"], d["sd"], d["y"], nbr, kind=kind, perms=perms, mode="geary",
                                       assumption="randomisation")
        assert isinstance(r, ResidualAutocorrPerm) and isinstance(g, ResidualGearyPerm) and r.n_perms == g.n_perms == 199
        assert r.I.shape == r.pval_greater.shape == g.C.shape == g.pval_less.shape == (100,) and g.variance.shape == (100,)
        pg, pl = r.pval_greater.cpu().numpy(), g.pval_less.cpu().numpy()
        print(kind, "planted", pg[c["planted"]].max(), pl[c["planted"]].max(), "others", pg[~c["planted"]].min(), pl[~c["planted"]].min())
        assert G.planted_found(pg, c["planted"]) and G.planted_found(pl, c["planted"])
        assert (r.z[torch.as_tensor(c["planted"]).cuda()] > 6).all()


# --- 9. the public path -----------------------------------------------------------------------------------------------

N_M, M_M, D_M, L_M = 300, 16, 40, 3


def _model_data():
    g = torch.Generator().manual_seed(91)
    X = 4.0 * torch.rand(N_M, 2, generator=g) - 2.0
    y = torch.randn(D_M, N_M, generator=g) + torch.sin(X[:, 0])[None, :]
    counts = torch.poisson(2.0 * torch.rand(D_M, N_M, generator=g), generator=g)
    return g, X.cuda(), y.cuda(), counts.cuda()


def _gp(g, X):
    import gpzoo.gp as GP
    import gpzoo.kernels as K
    gp = GP.WSVGP(K.NSF_RBF(L=L_M, lengthscale=2.0), dim=2, M=M_M, jitter=1e-2)
    gp.Z = nn.Parameter(X.cpu()[:M_M].clone(), requires_grad=False)
    gp.mu = nn.Parameter(0.3 * torch.randn(L_M, M_M, generator=g))
    gp.Lu = nn.Parameter(0.05 * torch.randn(L_M, M_M, M_M, generator=g) - 0.5 * torch.eye(M_M))
    return gp


def _same(a, b):
    return type(a) is type(b) and all((x is None and z is None) or (torch.equal(x, z) if isinstance(x, torch.Tensor) else x == z)
                                      for x, z in zip(a, b))


IDX = torch.tensor([5, 299, 0, 77, 31, 64, 63, 100, 12, 90, 41, 250, 130])


def _selections(X):
    idx = IDX.cuda()
    mask = torch.zeros(N_M, dtype=torch.bool, device="cuda")
    mask[::3] = True
    return (None, X), (idx, X[idx]), (mask, X[mask])


def test_rsf_methods_equal_the_hand_assembled_call():
    from gpzoo.likelihoods import RSF, ResidualAutocorr, ResidualGearyPerm, SparseExpression, SparseCounts, gaussian_residual_autocorr
    from gpzoo.likelihoods import model_residual_autocorr
    from gpzoo.likelihoods import _noise_sd
    from gpzoo_amd import ops
    g, X, y, _ = _model_data()
    model = RSF(_gp(g, X), y.cpu(), L=L_M)
    model.W = nn.Parameter(torch.randn(D_M, L_M, generator=g))
    model = model.cuda()
    for idx, Xb in _selections(X):
        yb = y if idx is None else y[:, idx]
        kw = {} if idx is None else dict(idx=idx)
        with torch.no_grad():
            qF = model.gp(X=Xb)[0]
            hand_args = ([qF], [model.W], model.b, _noise_sd(model.noise), yb, ops.spatial_knn(Xb, 6))
        for kind in G.KINDS:
            r = model_residual_autocorr(model, X, yb, kind=kind, **kw)
            assert isinstance(r, ResidualAutocorr) and all(t.dtype == torch.float64 and not t.requires_grad for t in r)
            assert r.I.shape == (D_M,) and _same(r, gaussian_residual_autocorr(*hand_args, kind=kind))
            assert _same(r, model_residual_autocorr(model, X, yb, kind=kind, graph=ops.spatial_knn(Xb, 6), **kw))
            genes = [7, 0, 39, 7]
            rows = model.residuals(X, yb, genes, kind=kind, **kw)
            full = ops.gaussian_residuals(qF.mean, qF.scale, model.W, model.b, _noise_sd(model.noise), yb, kind=kind)
            assert rows.shape == (4, Xb.shape[0]) and torch.equal(rows, full.T[genes])
        p = model_residual_autocorr(model, X, yb, mode="geary", assumption="randomisation", n_perms=9, seed=3, return_sims=True, **kw)
        hand = gaussian_residual_autocorr(*hand_args, mode="geary", assumption="randomisation", n_perms=9, seed=3, return_sims=True)
        assert isinstance(p, ResidualGearyPerm) and p.sims.shape == (D_M, 9) and _same(p, hand)
    assert all(q.grad is None for q in model.parameters())
    # held-out coordinates run, and the predictive kind differs there; a SparseExpression gives the dense array's bits
    Xh = 4.0 * torch.rand(50, 2, generator=g).cuda() - 2.0
    yh = torch.randn(D_M, 50, generator=g).cuda()
    a, b = model_residual_autocorr(model, Xh, yh), model_residual_autocorr(model, Xh, yh, kind="predictive")
    assert a.I.shape == (D_M,) and torch.isfinite(a.I).all() and not torch.equal(a.I, b.I)
    v = torch.relu(y)
    expr = SparseExpression(SparseCounts(v), v.double().mean(dim=1))
    assert _same(model_residual_autocorr(model, X, expr), model_residual_autocorr(model, X, expr.to_dense()))


def test_fa_methods_equal_the_hand_assembled_call():
    from gpzoo.gp import GaussianPrior
    from gpzoo.likelihoods import FA, ResidualAutocorr, gaussian_residual_autocorr, model_residual_autocorr, _noise_sd
    from gpzoo_amd import ops
    g, X, y, _ = _model_data()
    model = FA(GaussianPrior(y.cpu(), L=L_M), y.cpu(), L=L_M).cuda()
    for idx, Xb in _selections(X):
        yb = y if idx is None else y[:, idx]
        kw = {} if idx is None else dict(idx=idx)
        with torch.no_grad():
            qF = (model.prior() if idx is None else model.prior.forward_batched(idx))[0]
        r = model_residual_autocorr(model, X, yb, **kw)
        hand = gaussian_residual_autocorr([qF], [model.W], model.b, _noise_sd(model.noise), yb, ops.spatial_knn(Xb, 6))
        assert isinstance(r, ResidualAutocorr) and _same(r, hand)
        rows = model.residuals(X, yb, [3, 1], kind="response", **kw)
        full = ops.gaussian_residuals(qF.mean, qF.scale, model.W, model.b, _noise_sd(model.noise), yb, kind="response")
        assert torch.equal(rows, full.T[[3, 1]])
    with pytest.raises(ValueError, match="fitted spots"):
        model_residual_autocorr(model, X[:50], y[:, :50])


@pytest.mark.parametrize("likelihood", ["poisson", "nb"])
def test_pnmf_methods_equal_the_hand_assembled_call(likelihood):
    from gpzoo.gp import GaussianPrior
    from gpzoo.likelihoods import PNMF, ResidualAutocorr, model_residual_autocorr, residual_autocorr
    from gpzoo_amd import ops
    sp = torch.nn.functional.softplus
    g, X, _, counts = _model_data()
    model = PNMF(GaussianPrior(counts.cpu(), L=L_M), counts.cpu(), L=L_M, likelihood=likelihood)
    model.V = nn.Parameter(0.5 * torch.randn(N_M, generator=g))
    if likelihood == "nb":
        model.theta = nn.Parameter(2.0 * torch.randn(D_M, generator=g))
    model = model.cuda()
    theta = sp(model.theta.detach()) if likelihood == "nb" else None
    for idx, Xb in _selections(X):
        yb = counts if idx is None else counts[:, idx]
        kw = {} if idx is None else dict(idx=idx)
        with torch.no_grad():
            qF = (model.prior() if idx is None else model.prior.forward_batched(idx))[0]
            Vh = sp(model.V) if idx is None else sp(model.V)[idx]
        for kind in ("pearson", "deviance"):
            r = model_residual_autocorr(model, X, yb, kind=kind, **kw)
            hand = residual_autocorr([qF], [sp(model.W)], Vh, yb, ops.spatial_knn(Xb, 6), theta_pos=theta, kind=kind)
            assert isinstance(r, ResidualAutocorr) and _same(r, hand)
            rows = model.residuals(X, yb, [3, 1], kind=kind, **kw)
            full = ops.count_residuals(qF.mean, qF.scale, sp(model.W), Vh, yb, theta_pos=theta, kind=kind)
            assert torch.equal(rows, full.T[[3, 1]])
    if likelihood == "nb":                                    # scored under its theta
        assert _same(model_residual_autocorr(model, X, counts), model_residual_autocorr(model, X, counts, family="nb"))
        assert not torch.equal(model_residual_autocorr(model, X, counts, family="poisson").I, model_residual_autocorr(model, X, counts).I)
