"""CPU: the Matern-1/2 and Matern-5/2 kernels' oracle against the reference's own numbers, and their public surface.

tests/matern_oracle.py is pinned here against the fixtures tests/golden/make_matern_golden.py wrote by running the
reference with ``batched_Matern32`` subclasses whose ``covariance`` is the nu = 1/2 / nu = 5/2 closed form; the GPU
tests (tests/test_hip_matern_family.py) then check the HIP kernels against both."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import matern_oracle as MO
from helpers import GOLDEN, load_case
from oracle import svgp_oracle as O

from gpzoo.kernels import batched_Matern12, batched_Matern32, batched_Matern52     # noqa: E402  (the feature under test)

KINDS = ("matern12", "matern52")
CLASSES = {"matern12": batched_Matern12, "matern52": batched_Matern52}
CASES = [f"extra_{k}_{g}_{t}" for k in KINDS for g in ("wsvgp", "svgp") for t in ("f64", "f32")]


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_reference(name):
    """Every stored array, at test_oracle_golden.py's tolerances for the existing oracle."""
    c = load_case(name)
    dt = c["X"].dtype
    assert c["kind"] in KINDS and c["X"].shape == (160, 2) and c["Z"].shape == (36, 2) and c["mu"].shape == (3, 36)
    tight = dict(rtol=1e-10, atol=1e-12) if dt == torch.float64 else dict(rtol=2e-5, atol=2e-6)
    loose = tight if dt == torch.float64 else dict(rtol=1e-3, atol=1e-4)
    p = MO.parts(c["kind"], c["whitened"], c["X"], c["Z"], c["sigma"], c["lengthscale"], c["mu"], c["Lu_raw"], c["jitter"])
    torch.testing.assert_close(p["Kzx"], c["Kzx"], **tight)
    torch.testing.assert_close(p["Kzz_jit"], c["Kzz_jit"], **tight)
    torch.testing.assert_close(O.kernel_diag(c["sigma"], 160).reshape(c["Kxx"].shape), c["Kxx"], **tight)
    torch.testing.assert_close(p["chol"], c["chol"], **tight)
    torch.testing.assert_close(p["Lu"], c["Lu"], **tight)
    torch.testing.assert_close(p["mean"], c["mean"], **loose)
    torch.testing.assert_close(p["scale"], c["scale"], **loose)
    torch.testing.assert_close(p["kl"].reshape(c["kl"].shape), c["kl"], **loose)
    e, _, _ = MO.elbo_eval(c["kind"], c["whitened"], c["X"], c["y"], c["Z"], c["sigma"], c["lengthscale"], c["mu"],
                           c["Lu_raw"], c["jitter"], c["noise_sd"])
    assert float(e) == pytest.approx(c["elbo"], rel=1e-10 if dt == torch.float64 else 1e-5)
    # the reference's autograd gradients of -ELBO (its grad_Z is NaN and is not stored; the oracle's is finite)
    g = MO.grads(c["kind"], c["whitened"], c["X"], c["y"], c["Z"], c["sigma"], c["lengthscale"], c["mu"], c["Lu_raw"],
                 c["jitter"], c["noise_sd"])
    assert "grad_Z" not in c and torch.isfinite(g["grad_Z"]).all()
    for k in ("grad_mu", "grad_Lu", "grad_sigma", "grad_lengthscale"):
        sc = float(c[k].abs().max())
        tol = dict(rtol=1e-8, atol=1e-10 * sc) if dt == torch.float64 else dict(rtol=1e-3, atol=1e-3 * sc)
        torch.testing.assert_close(g[k], c[k], msg=lambda m: f"{k}: {m}", **tol)


def test_oracle_kernel_matrices():
    z = np.load(os.path.join(GOLDEN, "extra_matern_kernels_only.npz"), allow_pickle=False)
    for tag, dt, tol in (("f64", torch.float64, 1e-11), ("f32", torch.float32, 2e-5)):
        X, Z = torch.from_numpy(z[f"{tag}_X"]), torch.from_numpy(z[f"{tag}_Z"])
        assert X.shape == (96, 2) and Z.shape == (77, 2)
        vec = lambda *v: torch.tensor(v, dtype=dt)                    # noqa: E731
        sc = lambda v: torch.tensor(v).to(dt)                          # noqa: E731  (fp32 python constants cast by Module.to)
        for kind in KINDS:
            K = MO.kernel_matrix(kind, Z, X, vec(1.0, 0.8, 1.3), vec(2.5, 4.0, 6.0))
            torch.testing.assert_close(K, torch.from_numpy(z[f"{tag}_{kind}_vec"]), rtol=tol, atol=tol)
            K = MO.kernel_matrix(kind, Z, X, sc(0.9), sc(2.0))
            torch.testing.assert_close(K, torch.from_numpy(z[f"{tag}_{kind}_scalar"]), rtol=tol, atol=tol)
            K = MO.kernel_matrix(kind, Z, Z, sc(0.9), sc(2.0))
            torch.testing.assert_close(K, torch.from_numpy(z[f"{tag}_{kind}_zz"]), rtol=tol, atol=tol)
            assert torch.equal(torch.diagonal(K), (sc(0.9) ** 2).expand(77))


def test_fixture_points_are_separated():
    """No pair of distinct points closer than 1e-3 min(lengthscale): the fixtures do not depend on the ill-conditioned
    fp32 unit vector of the nu = 1/2 gradient (asserted by the generator; re-checked on what is committed)."""
    sets = [(load_case(n)["X"], load_case(n)["Z"], 2.5) for n in CASES]
    z = np.load(os.path.join(GOLDEN, "extra_matern_kernels_only.npz"), allow_pickle=False)
    sets += [(torch.from_numpy(z[f"{t}_X"]), torch.from_numpy(z[f"{t}_Z"]), 2.0) for t in ("f64", "f32")]
    for X, Z, ell in sets:
        P = torch.cat([X, Z]).double()
        d = torch.cdist(P, P) + torch.diag(torch.full((len(P),), float("inf"), dtype=torch.float64))
        assert float(d.min()) >= 1e-3 * ell


@pytest.mark.parametrize("kind", KINDS)
def test_public_surface_equals_matern32(kind):
    import gpzoo_amd.kernels as impl
    cls = CLASSES[kind]
    assert cls is getattr(impl, cls.__name__)
    assert inspect.signature(cls.__init__) == inspect.signature(batched_Matern32.__init__)
    assert inspect.signature(cls.forward) == inspect.signature(batched_Matern32.forward)
    assert inspect.signature(cls.covariance) == inspect.signature(batched_Matern32.covariance)
    k = cls()
    assert list(k.state_dict()) == ["sigma", "lengthscale"] == list(batched_Matern32().state_dict())
    assert float(k.sigma) == 1.0 and float(k.lengthscale) == 2.0 and k.sigma.dim() == 0
    k = cls(sigma=0.7, lengthscale=3.5)
    assert float(k.sigma) == pytest.approx(0.7) and float(k.lengthscale) == pytest.approx(3.5)


@pytest.mark.parametrize("kind", KINDS)
def test_covariance_method_is_the_closed_form(kind):
    g = torch.Generator().manual_seed(3)
    k = CLASSES[kind](sigma=0.9, lengthscale=2.0).double()
    for d in (1, 2, 4):
        x1, x2 = torch.randn(d, generator=g, dtype=torch.float64), torch.randn(d, generator=g, dtype=torch.float64)
        ref = MO.covariance(kind, x1, x2, k.sigma.detach(), k.lengthscale.detach())
        torch.testing.assert_close(k.covariance(x1, x2).detach(), ref, rtol=1e-14, atol=0)
    assert float(k.covariance(x1, x1)) == float(k.sigma.detach() ** 2)
    kv = CLASSES[kind]()
    kv.sigma = torch.nn.Parameter(torch.tensor([1.0, 0.8, 1.3], dtype=torch.float64))
    kv.lengthscale = torch.nn.Parameter(torch.tensor([2.5, 4.0, 6.0], dtype=torch.float64))
    ref = MO.covariance(kind, x1, x2, kv.sigma.detach(), kv.lengthscale.detach())
    assert ref.shape == (3,)
    torch.testing.assert_close(kv.covariance(x1, x2).detach(), ref, rtol=1e-14, atol=0)


@pytest.mark.parametrize("kind", KINDS)
def test_user_defined_covariance_is_refused(kind):
    """Only the shipped closed forms have HIP kernels: an override is refused, the unmodified class passes that check
    (and then asks for device tensors)."""
    from gpzoo_amd.kernels import kernel_spec
    cls = CLASSES[kind]

    class Mine(cls):
        def covariance(self, x1, x2):
            return (self.sigma ** 2) * torch.exp(-((x1 - x2) ** 2).sum())

    X = torch.zeros(4, 2)
    with pytest.raises(NotImplementedError, match="user-defined"):
        Mine()(X, X)
    with pytest.raises(NotImplementedError, match="user-defined"):
        kernel_spec(Mine(), X, 2)
    patched = cls()
    patched.covariance = lambda x1, x2: x1.sum()
    with pytest.raises(NotImplementedError, match="user-defined"):
        patched(X, X)

    class Renamed(cls):          # a subclass that keeps the shipped covariance is the shipped kernel
        pass

    for k in (cls(), Renamed()):
        k._check_covariance()
        with pytest.raises(Exception) as ei:
            k(X, X)
        assert not isinstance(ei.value, NotImplementedError) and re.search("cuda|CUDA|device|GPU", str(ei.value))
    assert cls()(X, X, diag=True).shape == (4,)


def test_abi_constants():
    from gpzoo_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "gpzoo_hip.h")).read()
    enum = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"\b(GPZ_KERNEL_[A-Z0-9_]+)\s*=\s*(\d+)", text))
    assert enum["GPZ_KERNEL_MATERN12"] == _lib.KERNEL_MATERN12 == 4
    assert enum["GPZ_KERNEL_MATERN52"] == _lib.KERNEL_MATERN52 == 5
    assert (enum["GPZ_KERNEL_RBF"], enum["GPZ_KERNEL_MATERN32"], enum["GPZ_KERNEL_MGGP_RBF"], enum["GPZ_KERNEL_DISTANCE"]) == (0, 1, 2, 3)
    assert sorted(enum.values()) == list(range(6))
    assert re.search(r"#define\s+GPZ_VERSION\s+212\b", text)
    assert batched_Matern12._kind == 4 and batched_Matern52._kind == 5


@pytest.mark.parametrize("kind", KINDS)
def test_configs_accept_the_new_kinds(kind):
    from gpzoo_amd.configs import kernel_for_config
    from gpzoo_amd.synthetic import CONFIGS, make_config
    c = make_config(3, N=50, M=8, L=2, kind=kind)
    base = make_config(3, N=50, M=8, L=2)
    assert c["kind"] == kind and base["kind"] == "matern32" == CONFIGS[3]["kind"]
    for k in ("X", "Z", "y", "mu", "Lu_raw", "sigma", "lengthscale"):
        assert torch.equal(c[k], base[k])
    assert type(kernel_for_config(c)) is CLASSES[kind]
    assert make_config(3, N=50, M=8, L=2, kind="matern32")["kind"] == "matern32"
    with pytest.raises(ValueError):
        make_config(2, N=50, M=8, L=2, kind=kind)
    with pytest.raises(ValueError):
        make_config(3, N=50, M=8, L=2, kind="rbf")
