"""CPU: the surface of the negative-binomial likelihood -- the C entries, the ``likelihood=`` / ``theta0=`` keywords of the
count models (Poisson stays the default and keeps the reference's parameters), and the host-side refusals."""
import inspect
import json
import os

import pytest
import torch

from conftest import ROOT
from helpers import GOLDEN

NEW_SYMBOLS = ("gpz_nb_nsf", "gpz_nb_nsf_workspace_bytes")
COUNT_MODELS = ("PNMF", "NSF2", "NSF", "MGGP_NSF", "Hybrid_NSF2", "Hybrid_NSF_Exact", "Hybrid_NSF")
D, N = 7, 11


def builders(**kw):
    import gpzoo.gp as g
    import gpzoo.kernels as k
    import gpzoo.likelihoods as li
    y = torch.ones(D, N)
    gp_of = lambda cls, kern, **a: cls(kern, dim=2, M=6, **a)  # noqa: E731
    return {
        "PNMF": lambda: li.PNMF(g.GaussianPrior(y, L=3), y, L=3, **kw),
        "NSF2": lambda: li.NSF2(gp_of(g.WSVGP, k.NSF_RBF(L=3)), y, L=3, **kw),
        "NSF": lambda: li.NSF(gp_of(g.WSVGP, k.NSF_RBF(L=3)), y, L=3, **kw),
        "MGGP_NSF": lambda: li.MGGP_NSF(gp_of(g.MGGP_WSVGP, k.MGGP_NSF_RBF(L=3, n_groups=3), n_groups=3), y, L=3, **kw),
        "Hybrid_NSF2": lambda: li.Hybrid_NSF2(gp_of(g.WSVGP, k.NSF_RBF(L=3)), g.GaussianPrior(y, L=2), y, L=3, T=2, **kw),
        "Hybrid_NSF_Exact": lambda: li.Hybrid_NSF_Exact(gp_of(g.WSVGP, k.NSF_RBF(L=3)), g.GaussianPrior(y, L=2), y, L=3, T=2, **kw),
        "Hybrid_NSF": lambda: li.Hybrid_NSF(gp_of(g.WSVGP, k.NSF_RBF(L=3)), y, L=3, non_spatial_factors=2, **kw),
    }


def reference_keys():
    with open(os.path.join(GOLDEN, "state_dict_keys.json")) as f:
        return json.load(f)


def test_new_entries_are_declared_and_bound():
    from gpzoo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpzoo_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in hdr and name in _lib.exported_symbols()
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
    from gpzoo_amd import ops
    assert callable(ops.nb_nsf)
    import gpzoo.likelihoods as li
    assert callable(li.nb_expected_loglik) and issubclass(li._NBLogLik, torch.autograd.Function)


@pytest.mark.parametrize("name", COUNT_MODELS)
def test_poisson_default_keeps_the_reference_parameters(name):
    ref = reference_keys()[name]
    for make in (builders()[name], builders(likelihood="poisson")[name]):
        m = make()
        assert m.likelihood == "poisson" and not hasattr(m, "theta")
        got = {k: [list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()}
        assert got == ref


@pytest.mark.parametrize("name", COUNT_MODELS)
def test_nb_adds_theta_only(name):
    ref = reference_keys()[name]
    m = builders(likelihood="nb", theta0=3.5)[name]()
    sd = m.state_dict()
    assert set(sd) == set(ref) | {"theta"}
    assert {k: [list(v.shape), str(v.dtype)] for k, v in sd.items() if k != "theta"} == ref
    assert isinstance(m.theta, torch.nn.Parameter) and m.theta.shape == (D,) and m.theta.requires_grad
    torch.testing.assert_close(torch.nn.functional.softplus(m.theta.detach()), torch.full((D,), 3.5), rtol=1e-4, atol=0)
    d = builders(likelihood="nb")[name]()
    torch.testing.assert_close(torch.nn.functional.softplus(d.theta.detach()), torch.full((D,), 10.0), rtol=1e-4, atol=0)


@pytest.mark.parametrize("name", COUNT_MODELS)
def test_unknown_likelihood_is_refused(name):
    with pytest.raises(ValueError, match="gamma"):
        builders(likelihood="gamma")[name]()


def test_new_constructor_keywords_are_trailing_and_have_defaults():
    import gpzoo.likelihoods as li
    for name in COUNT_MODELS + ("PoissonFactorization",):
        ps = list(inspect.signature(getattr(li, name).__init__).parameters.values())
        assert [p.name for p in ps[-2:]] == ["likelihood", "theta0"], name
        assert ps[-2].default == "poisson" and ps[-1].default == 10.0, name


def test_forward_builds_torchs_negative_binomial():
    """pY of an NB model on the CPU pieces that need no kernel: the distribution's parameters from a given rate."""
    import gpzoo.likelihoods as li
    m = builders(likelihood="nb", theta0=2.0)["NSF"]()
    rate = torch.rand(3, D, N) + 0.1
    pY = li._count_dist(m, rate)
    assert isinstance(pY, torch.distributions.NegativeBinomial)
    torch.testing.assert_close(pY.mean, rate, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(pY.variance, rate + rate ** 2 / 2.0, rtol=1e-4, atol=1e-6)
    assert isinstance(li._count_dist(builders()["NSF"](), rate), torch.distributions.Poisson)


def test_workspace_query_refuses_bad_extents_on_the_host():
    from gpzoo_amd import _lib
    lib = _lib.load()
    assert lib.gpz_nb_nsf_workspace_bytes(100, 10, 20, 3) > 0
    assert lib.gpz_nb_nsf_workspace_bytes(100, 10, 65, 3) == 0
    assert b"65 factors unsupported" in lib.gpz_last_error()
    assert lib.gpz_nb_nsf_workspace_bytes(100, 10, 20, 33) == 0
    assert b"33 samples per call unsupported" in lib.gpz_last_error()
    assert lib.gpz_nb_nsf_workspace_bytes(0, 10, 20, 3) == 0
    # nothing of D x N elements: ten times the spots and genes cost far less than a hundred times the bytes of y would
    big = lib.gpz_nb_nsf_workspace_bytes(7000, 17702, 20, 3)
    assert big < 0.5 * 4 * 7000 * 17702


def test_null_pointers_are_refused_before_any_launch():
    from gpzoo_amd import _lib
    lib = _lib.load()
    rc = lib.gpz_nb_nsf(None, None, None, None, None, None, None, 10, 4, 3, 1, 1, None, None, None, None, None, None, None, 0,
                        None)
    assert rc < 0 and b"gpz_nb_nsf: null pointer" in lib.gpz_last_error()


def test_sharded_step_refuses_an_nb_model():
    from gpzoo_amd import parallel
    m = builders(likelihood="nb")["NSF"]()
    with pytest.raises(NotImplementedError, match="Poisson likelihood only"):
        parallel.sharded_nsf_step(m, None, None, None, None, None, 3)
