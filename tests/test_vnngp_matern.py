"""CPU: the VNNGP-over-Matern oracle (tests/vnngp_matern_oracle.py) against the reference's own VNNGP run with Matern-1/2,
-3/2 and -5/2 kernels (tests/golden/make_vnngp_matern_golden.py -> extra_vnngp_matern*.npz), every stored array at rtol
1e-5: the GPU tests compare the HIP path with this oracle, so this file ties the oracle to the reference."""
import pytest
import torch

import vnngp_matern_oracle as VO
from helpers import load_case

CASES = [f"extra_vnngp_{kind}_{tag}" for kind in VO.KINDS for tag in ("f64", "f32")]


@pytest.fixture(scope="module", params=CASES)
def case(request):
    """(fixture, oracle outputs and gradients on the fixture's inputs, in the fixture's own precision)."""
    c = load_case(request.param)
    d = {k: c[k] for k in ("X", "y", "Z", "sigma", "lengthscale", "mu", "Lu_raw")}
    K = int(c["K"])
    mean, scale, idx, Lu, chol = VO.vnngp_moments(c["kind"], d["X"], d["Z"], d["sigma"], d["lengthscale"], d["mu"],
                                                  d["Lu_raw"], c["jitter"], K)
    g = VO.grads(c["kind"], d["X"], d["y"], d["Z"], d["sigma"], d["lengthscale"], d["mu"], d["Lu_raw"], c["jitter"], K,
                 c["noise_sd"])
    return c, dict(mean=mean, scale=scale, idx=idx, Lu=Lu, chol=chol, **g)


def test_fixture_contents(case):
    c, _ = case
    assert c["kind"] in VO.KINDS and int(c["K"]) == 10 and tuple(c["idx"].shape) == (c["X"].shape[0], 10)
    assert "grad_Z" not in c                       # NaN in the reference: not stored
    for k, v in c.items():
        if isinstance(v, torch.Tensor) and v.is_floating_point():
            assert bool(torch.isfinite(v).all()), k
    assert int(c["n_clamped"]) == 0 and float(((c["scale"].double() ** 2 - 5e-2).abs() / 5e-2).min()) > 1e-6


def test_oracle_neighbour_table_equals_reference(case):
    c, o = case
    assert torch.equal(o["idx"], c["idx"])


@pytest.mark.parametrize("key", ["mean", "scale", "Lu", "chol", "loss", "grad_mu", "grad_Lu", "grad_sigma", "grad_lengthscale"])
def test_oracle_matches_reference(case, key):
    """rtol 1e-5 with atol = 1e-5 max|ref| in both precisions: the oracle runs in the fixture's precision (its forward is
    the reference's op sequence; only the order of autograd's sums differs)."""
    c, o = case
    ref = c[key]
    torch.testing.assert_close(o[key].reshape(ref.shape).to(ref.dtype), ref, rtol=1e-5, atol=1e-5 * float(ref.abs().max()))


def test_oracle_grad_Z_is_finite_where_the_reference_has_nan(case):
    _, o = case
    assert bool(torch.isfinite(o["grad_Z"]).all()) and float(o["grad_Z"].abs().max()) > 0


@pytest.mark.parametrize("kind", VO.KINDS)
def test_oracle_scalar_parameters_and_caller_table(kind):
    """Scalar parameters give (N,) moments equal to the one-latent case; ``idx=`` replaces the argsort."""
    g = torch.Generator().manual_seed(3)
    X = (torch.rand(50, 2, generator=g, dtype=torch.float64) - 0.5) * 10
    Z = (torch.rand(12, 2, generator=g, dtype=torch.float64) - 0.5) * 10
    mu, Lu = torch.randn(12, generator=g, dtype=torch.float64), 0.1 * torch.randn(12, 12, generator=g, dtype=torch.float64)
    s, ell = torch.tensor(0.9, dtype=torch.float64), torch.tensor(2.0, dtype=torch.float64)
    m0, s0, idx, _, ch0 = VO.vnngp_moments(kind, X, Z, s, ell, mu, Lu, 1e-2, 4)
    m1, s1, idx1, _, ch1 = VO.vnngp_moments(kind, X, Z, s.reshape(1), ell.reshape(1), mu[None], Lu[None], 1e-2, 4, idx=idx)
    assert m0.shape == (50,) and ch0.shape == (12, 12) and torch.equal(idx, idx1)
    torch.testing.assert_close(m1[0], m0, rtol=1e-12, atol=0)
    torch.testing.assert_close(s1[0], s0, rtol=1e-12, atol=0)
