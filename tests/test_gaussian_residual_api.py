"""CPU: the surface of the Gaussian residual diagnostics -- the C symbols, the signatures of the ops and of
gpzoo.likelihoods, every refusal that needs no device (each with its message), and the flags of examples/rsf_synthetic.py."""
import importlib.util
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

SYMBOLS = ("gpz_gaussian_residual_plan", "gpz_gaussian_residuals", "gpz_gaussian_residuals_sparse", "gpz_gaussian_residual_stats",
           "gpz_gaussian_residual_stats_sparse", "gpz_gaussian_residual_perm", "gpz_gaussian_residual_perm_sparse")
N, D, L = 40, 6, 2


def _names(fn):
    return [(n, p.kind.name, p.default) for n, p in inspect.signature(fn).parameters.items()]


def test_the_seven_symbols_are_in_the_header_and_the_loader_table():
    from gpzoo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpzoo_hip.h")).read()
    declared = set(re.findall(r"\bint (gpz_[a-z0-9_]+)\s*\(", hdr))
    assert set(SYMBOLS) <= declared and set(SYMBOLS) <= set(_lib.exported_symbols())
    assert "#define GPZ_VERSION 212" in hdr


def test_the_plan_is_a_host_only_query_with_the_count_plans_numbers():
    from gpzoo_amd import ops
    g, c = ops.gaussian_residual_plan(7000, 17702, 20, 6, 100), ops.residual_autocorr_perm_plan(7000, 17702, 20, 6, 100)
    assert all(g[k] == c[k] for k in c) and g["factors_padded"] == 20 and g["spot_slices"] >= 1
    assert g["slab_genes"] * 7000 * 4 <= 256 << 20
    small = ops.gaussian_residual_plan(7000, 17702, 20)
    assert small["perm_batch"] == small["batches"] == 0 and small["partials_bytes"] < 1 << 20
    for args, msg in (((7000, 100, 65, 6), "65 factors unsupported"), ((7000, 100, 0, 6), "0 factors unsupported"),
                      ((7000, 100, 20, 33), "K = 33 neighbours"), ((6, 100, 20, 6), "K = 6 neighbours of 6 spots"),
                      ((1 << 31, 100, 20, 6), "indexed with 32 bits"), ((7000, 100, 20, 0, 5), "without a neighbour table"),
                      ((1 << 27, 100, 20, 6, 0, 5), "stored counts over"), ((7000, 100, 20, 6, 0, 0, 100), "slab_genes = 100")):
        with pytest.raises(ValueError, match=msg):
            ops.gaussian_residual_plan(*args)


def test_the_ops_signatures():
    from gpzoo_amd import ops
    e = inspect.Parameter.empty
    pk, ko = "POSITIONAL_OR_KEYWORD", "KEYWORD_ONLY"
    head = [(n, pk, e) for n in ("mean", "scale", "W", "b", "noise_sd", "y")]
    assert _names(ops.gaussian_residuals) == head + [("genes", pk, None), ("kind", pk, "pearson")]
    assert _names(ops.gaussian_residual_stats) == head + [("nbr", pk, e), ("genes", pk, None), ("kind", pk, "pearson"),
                                                          ("slab_genes", pk, 0)]
    assert _names(ops.gaussian_residual_autocorr_perm) == head + [
        ("nbr", pk, e), ("perms", pk, e), ("genes", pk, None), ("kind", pk, "pearson"), ("stat", ko, "moran"),
        ("return_sims", ko, False), ("perm_batch", ko, 0), ("slab_genes", ko, 0)]
    assert [n for n, _, _ in _names(ops.gaussian_residual_plan)] == ["B", "D", "Lt", "K", "P", "nnz", "slab_genes", "perm_batch"]
    assert ops.GAUSSIAN_RESIDUAL_KINDS == {"pearson": 0, "response": 1, "predictive": 2}


def test_the_likelihoods_signatures():
    import gpzoo.likelihoods as Lk
    e = inspect.Parameter.empty
    pk, ko = "POSITIONAL_OR_KEYWORD", "KEYWORD_ONLY"
    null = [("mode", ko, "moran"), ("assumption", ko, "normality"), ("n_perms", ko, None), ("seed", ko, 0), ("perms", ko, None),
            ("return_sims", ko, False)]
    assert _names(Lk.gaussian_residual_autocorr) == [(n, pk, e) for n in ("qF_list", "W_list", "b", "noise_sd", "y", "nbr")] + [
        ("kind", ko, "pearson"), ("slab_genes", ko, 0)] + null
    assert _names(Lk.gaussian_residuals) == [(n, pk, e) for n in ("qF_list", "W_list", "b", "noise_sd", "y", "genes")] + [
        ("kind", ko, "pearson")]
    for cls in (Lk.RSF, Lk.FA):
        assert _names(cls._residual_autocorr) == [("self", pk, e), ("X", pk, e), ("y", pk, e), ("idx", pk, None), ("kind", ko, "pearson"),
                                                  ("n_neighs", ko, 6), ("graph", ko, None)] + null + [("groupsX", ko, None)]
        assert _names(cls.residuals)[:5] == [("self", pk, e), ("X", pk, e), ("y", pk, e), ("genes", pk, e), ("idx", pk, None)]
    # the three models are scored through model_residual_autocorr, which also takes the count models that have the method
    assert _names(Lk.model_residual_autocorr) == [("model", pk, e), ("X", pk, e), ("y", pk, e), ("idx", pk, None),
                                                  ("keywords", "VAR_KEYWORD", e)]
    assert _names(Lk.PNMF._residual_autocorr) == _names(Lk.NSF.residual_autocorr)
    assert _names(Lk.PNMF.residuals) == _names(Lk.NSF.residuals)
    with pytest.raises(TypeError, match="model_residual_autocorr: Linear has no residual diagnostic"):
        Lk.model_residual_autocorr(torch.nn.Linear(1, 1), None, None)
    for doc in (Lk.gaussian_residual_autocorr.__doc__, inspect.getsource(Lk.gaussian_residual_autocorr)):
        assert "affine" in doc and "predictive" in doc


# --- refusals that need no device: models on the CPU, nothing is launched ---------------------------------------------

@pytest.fixture(scope="module")
def models():
    import gpzoo.gp as GP
    import gpzoo.kernels as K
    import gpzoo.likelihoods as Lk
    g = torch.Generator().manual_seed(0)
    y = torch.randn(D, N, generator=g)
    counts = torch.poisson(2.0 * torch.rand(D, N, generator=g), generator=g)
    X = torch.rand(N, 2, generator=g)
    rsf = Lk.RSF(GP.WSVGP(K.NSF_RBF(L=L, lengthscale=1.0), dim=2, M=8, jitter=1e-2), y, L=L)
    fa = Lk.FA(GP.GaussianPrior(y, L=L), y, L=L)
    pnmf = Lk.PNMF(GP.GaussianPrior(counts, L=L), counts, L=L)
    return dict(RSF=rsf, FA=fa, PNMF=pnmf, X=X, y=y, counts=counts)


@pytest.mark.parametrize("name", ["RSF", "FA"])
def test_gaussian_models_refuse_before_any_device_work(models, name):
    import gpzoo.likelihoods as Lk
    m, X, y, counts = models[name], models["X"], models["y"], models["counts"]
    with pytest.raises(ValueError, match=rf'{name}\.residual_autocorr: kind="deviance" is kind="pearson" for a Gaussian'):
        Lk.model_residual_autocorr(m, X, y, kind="deviance")
    with pytest.raises(ValueError, match=rf'{name}\.residuals: kind="deviance" is kind="pearson"'):
        m.residuals(X, y, [0], kind="deviance")
    with pytest.raises(ValueError, match=rf'{name}\.residual_autocorr: kind must be "pearson", "response" or "predictive", got \'anscombe\''):
        Lk.model_residual_autocorr(m, X, y, kind="anscombe")
    with pytest.raises(ValueError, match=rf"{name}\.residual_autocorr: mode='lisa' unknown"):
        Lk.model_residual_autocorr(m, X, y, mode="lisa")
    with pytest.raises(ValueError, match=rf"{name}\.residual_autocorr: assumption='bootstrap' unknown"):
        Lk.model_residual_autocorr(m, X, y, assumption="bootstrap")
    with pytest.raises(ValueError, match=rf"{name}\.residual_autocorr: assumption='randomisation' needs B >= 4 spots, got 3"):
        Lk.model_residual_autocorr(m, X, y[:, :3], idx=torch.tensor([0, 1, 2]), assumption="randomisation")
    sc = Lk.SparseCounts(counts)
    with pytest.raises(TypeError, match=rf"{name}\.residual_autocorr: a SparseCounts holds counts"):
        Lk.model_residual_autocorr(m, X, sc)
    with pytest.raises(TypeError, match=rf"{name}\.residuals: a SparseCounts holds counts"):
        m.residuals(X, sc, [0])
    with pytest.raises(TypeError, match=rf"{name}\.residual_autocorr: a TransposedCounts holds counts"):
        Lk.model_residual_autocorr(m, X, sc.T)
    view = Lk.SparseExpression(sc, torch.zeros(D))[:, torch.arange(10)]
    with pytest.raises(TypeError, match=rf"{name}\.residual_autocorr: a view y\[:, idx\]; the whole data set is needed"):
        Lk.model_residual_autocorr(m, X, view, idx=torch.arange(10))
    with pytest.raises(TypeError, match=rf"{name}\.residual_autocorr: y must be a dense"):
        Lk.model_residual_autocorr(m, X, y.numpy())


def test_pnmf_refuses_before_any_device_work(models):
    import gpzoo.likelihoods as Lk
    m, X, counts = models["PNMF"], models["X"], models["counts"]
    sc = Lk.SparseCounts(counts)
    expr = Lk.SparseExpression(sc, torch.zeros(D))
    with pytest.raises(TypeError, match=r"PNMF\.residual_autocorr: a SparseExpression holds real-valued expression"):
        Lk.model_residual_autocorr(m, X, expr)
    with pytest.raises(TypeError, match=r"PNMF\.residuals: a SparseExpression holds real-valued expression"):
        m.residuals(X, expr, [0])
    with pytest.raises(TypeError, match=r"PNMF\.residual_autocorr: a view y\[:, idx\]"):
        Lk.model_residual_autocorr(m, X, sc[:, torch.arange(10)], idx=torch.arange(10))
    with pytest.raises(ValueError, match=r'PNMF\.residual_autocorr: kind must be "pearson" or "deviance", got \'response\''):
        Lk.model_residual_autocorr(m, X, counts, kind="response")
    with pytest.raises(ValueError, match=r"PNMF\.residual_autocorr: mode='lisa' unknown"):
        Lk.model_residual_autocorr(m, X, counts, mode="lisa")
    with pytest.raises(ValueError, match=r"PNMF\.residual_autocorr: assumption='bootstrap' unknown"):
        Lk.model_residual_autocorr(m, X, counts, assumption="bootstrap")
    with pytest.raises(ValueError, match=r"PNMF\.residual_autocorr: assumption='randomisation' needs B >= 4 spots, got 3"):
        Lk.model_residual_autocorr(m, X, counts[:, :3], idx=torch.tensor([0, 1, 2]), assumption="randomisation")
    with pytest.raises(ValueError, match=r'PNMF\.deviance: family must be'):
        Lk.model_residual_autocorr(m, X, counts, family="gaussian")


def test_the_functions_refuse_before_any_device_work(models):
    import gpzoo.likelihoods as Lk
    from gpzoo_amd import ops
    from torch.distributions import Normal
    y, counts = models["y"], models["counts"]
    qF, W, b, sd = [Normal(torch.zeros(L, N), torch.ones(L, N))], [torch.zeros(D, L)], torch.zeros(D), torch.ones(D)
    nbr = torch.stack([(torch.arange(N) + 1) % N, (torch.arange(N) + 2) % N], dim=1)
    with pytest.raises(ValueError, match=r'gaussian_residual_autocorr: kind="deviance" is kind="pearson"'):
        Lk.gaussian_residual_autocorr(qF, W, b, sd, y, nbr, kind="deviance")
    with pytest.raises(ValueError, match=r"gaussian_residual_autocorr: mode='lisa' unknown"):
        Lk.gaussian_residual_autocorr(qF, W, b, sd, y, nbr, mode="lisa")
    with pytest.raises(TypeError, match=r"gaussian_residual_autocorr: a SparseCounts holds counts"):
        Lk.gaussian_residual_autocorr(qF, W, b, sd, Lk.SparseCounts(counts), nbr)
    with pytest.raises(ValueError, match=r"gaussian_residuals: genes \(a list of gene indices\) needed"):
        Lk.gaussian_residuals(qF, W, b, sd, y, None)
    m, s = qF[0].mean, qF[0].scale
    with pytest.raises(ValueError, match=r"gaussian_residual_stats: K = 33 neighbours unsupported"):
        ops.gaussian_residual_stats(m, s, W[0], b, sd, y, torch.zeros(N, 33, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"gaussian_residual_stats: slab_genes = 100"):
        ops.gaussian_residual_stats(m, s, W[0], b, sd, y, nbr, slab_genes=100)
    with pytest.raises(ValueError, match=r"gaussian_residual_stats: .* do not fit together"):
        ops.gaussian_residual_stats(m, s, W[0], b[:-1], sd, y, nbr)
    with pytest.raises(IndexError, match=r"gaussian_residuals: a gene index lies outside \[0, 6\)"):
        ops.gaussian_residuals(m, s, W[0], b, sd, y, genes=[0, 6])
    with pytest.raises(ValueError, match=r"gaussian_residual_autocorr_perm: stat 'lisa' unknown"):
        ops.gaussian_residual_autocorr_perm(m, s, W[0], b, sd, y, nbr, torch.arange(N)[None], stat="lisa")


def test_the_example_flags_parse():
    spec = importlib.util.spec_from_file_location("rsf_synthetic", os.path.join(ROOT, "examples", "rsf_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.parse_args([])
    assert a.residual_autocorr is False and a.residual_perms is None and a.residual_mode == "moran"
    a = mod.parse_args(["--residual-autocorr", "--residual-perms", "99", "--residual-mode", "geary", "--sparse-expression", "0.05"])
    assert a.residual_autocorr and a.residual_perms == 99 and a.residual_mode == "geary" and a.sparse_expression == 0.05
    with pytest.raises(SystemExit):
        mod.parse_args(["--residual-perms", "99"])
    with pytest.raises(SystemExit):
        mod.parse_args(["--residual-autocorr", "--residual-mode", "lisa"])
