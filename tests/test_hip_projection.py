"""GPU: gpz_kernel_gram (ops.kernel_gram) and project_factors_to_inducing against the torch fp64 oracle
(tests/projection_oracle.py) and the fixtures the notebook's composition produced on the reference's kernels -- never
against the code under test.

Tolerances.  G and b: the project's kernel-entry tolerances (tests/test_hip_kernel_entries.py) scaled to G's size -- fp64
rtol 1e-9, atol 1e-9 max diag(G); fp32 rtol 1e-4, atol 1e-4 max diag(G).  mu and alpha on the fixtures (cond(G) <= 1e4):
fp64 1e-7 of max|mu| (G good to 1e-12 leaves the error below 1e-8), fp32 1e-3 of max|mu| (helpers.rtol_for)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import helpers
import projection_cases as PC
import projection_oracle as PO
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES = PC.cases()


def golden(name):
    return np.load(os.path.join(GOLDEN, f"extra_projection_{name}.npz"))


def tdtype(name):
    return torch.float32 if name == "f32" else torch.float64


def spec_of(kind, sigma, ell, dt, per_latent):
    from gpzoo_amd import ops
    s, e = torch.as_tensor(sigma).reshape(-1).to(dt).cuda(), torch.as_tensor(ell).reshape(-1).to(dt).cuda()
    return ops.KernelSpec(PO.KIND_CODE[kind], s, e, per_latent)


def run_gram(kind, dat, dt, per_latent, jitter):
    from gpzoo_amd import ops
    spec = spec_of(kind, dat["sigma"], dat["lengthscale"], dt, per_latent)
    Z, X, F = (torch.as_tensor(dat[k]).to(dt).cuda() for k in ("Z", "X", "F"))
    G, b = ops.kernel_gram(spec, Z, X, F, jitter)
    return G, b


def make_kernel(cls, sigma, ell, L, dt):
    from gpzoo import kernels as K
    s, e = torch.as_tensor(sigma).to(dt), torch.as_tensor(ell).to(dt)
    if cls == "NSF_RBF":
        k = K.NSF_RBF(L=L)
        k.sigma.data, k.lengthscale.data = s.reshape(L, 1, 1).clone(), e.reshape(L, 1, 1).clone()
    else:
        k = getattr(K, cls)()
        k.sigma.data, k.lengthscale.data = s.clone(), e.clone()
    return k


def assert_close(got, want, tol, scale, what):
    got, want = got.double().cpu(), want.double()
    err = (got - want).abs()
    bad = err > tol * want.abs() + tol * scale
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} entries off, max error {float(err.max()):.3e} (scale {scale:.3e})"


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_gram_and_rhs_match_the_oracle(case):
    p = PC.plan_of(case)
    dat = PC.data_of(case, p["N"])
    dt = tdtype(case["dtype"])
    jitter = 1e-5
    G, b = run_gram(case["kind"], dat, dt, case["per_latent"], jitter)
    o = PO.project(case["kind"], dat["Z"], dat["X"], dat["F"], torch.as_tensor(dat["sigma"]), torch.as_tensor(dat["lengthscale"]),
                   jitter=jitter)
    n, R, M = (case["L"], 1, case["M"]) if case["per_latent"] else (1, case["L"], case["M"])
    assert G.shape == (n, M, M) and b.shape == (n, R, M) and G.dtype == b.dtype == torch.float64
    tol = 1e-4 if case["dtype"] == "f32" else 1e-9
    scale = float(torch.diagonal(o["G"], dim1=-2, dim2=-1).max())
    bscale = float(o["b"].abs().max())
    Gc = G.cpu()
    assert torch.equal(Gc, Gc.transpose(-1, -2)), "G is not exactly symmetric"
    t = p["tile"]
    assert_close(G[:, :t, :t], o["G"][:, :t, :t], tol, scale, "G, first tile")
    assert_close(b[:, :, :t], o["b"][:, :, :t], tol, bscale, "b, first tile")
    if M > t:
        assert_close(G[:, t:, :], o["G"][:, t:, :], tol, scale, "G, rows beyond the first tile")
        assert_close(b[:, :, t:], o["b"][:, :, t:], tol, bscale, "b, rows beyond the first tile")
    # the diagonal carries the jitter: without it the matrix is the plain product
    K3 = o["Kzx"] if case["per_latent"] else o["Kzx"][None]
    plain = torch.diagonal(K3 @ K3.transpose(-1, -2), dim1=-2, dim2=-1)
    got = torch.diagonal(Gc, dim1=-2, dim2=-1) - plain
    assert float((got - jitter).abs().max()) <= tol * scale
    if p["n_splits"] > 1:
        # what the columns beyond the first split add, on its own: a dropped split is named here
        c = p["cols_per_split"]
        first, rest = K3[:, :, :c], K3[:, :, c:]
        assert_close(G - (first @ first.transpose(-1, -2) + jitter * torch.eye(M, dtype=torch.float64)).cuda(),
                     rest @ rest.transpose(-1, -2), tol, scale, "G, columns of X beyond the first split")
        F = torch.as_tensor(dat["F"]).double()
        Fb = F[:, None, :] if case["per_latent"] else F[None]
        assert_close(b - (Fb[:, :, :c] @ first.transpose(-1, -2)).cuda(), Fb[:, :, c:] @ rest.transpose(-1, -2), tol, bscale,
                     "b, columns of X beyond the first split")


def test_the_jitter_lands_on_the_diagonal_only():
    case = next(c for c in CASES if c["name"] == "splits_f64")
    p = PC.plan_of(case)
    dat = PC.data_of(case, p["N"])
    G0, b0 = run_gram(case["kind"], dat, torch.float64, True, 0.0)
    G1, b1 = run_gram(case["kind"], dat, torch.float64, True, 0.5)
    eye = torch.eye(case["M"], dtype=torch.float64, device="cuda")
    assert torch.equal(G1, G0 + 0.5 * eye) and torch.equal(b0, b1)


@pytest.mark.parametrize("name", sorted(PC.GOLDENS))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mu_and_alpha_match_the_fixtures_and_the_oracle(name, dtype):
    from gpzoo.utilities import project_factors_to_inducing
    z = golden(name)
    N, M, L, frac, cls, per_latent = PC.GOLDENS[name]
    dt = tdtype(dtype)
    jitter, kzz_jitter = float(z["jitter"]), 1e-4
    kernel = make_kernel(cls, z["sigma"], z["lengthscale"], L, dt)
    Z, X, F = (z[k].astype(PC.np_dtype(dtype)) for k in ("Z", "X", "F"))
    o = PO.project(PC.GOLDEN_KIND[cls], z["Z"], z["X"], z["F"], torch.as_tensor(z["sigma"]), torch.as_tensor(z["lengthscale"]),
                   jitter=jitter, kzz_jitter=kzz_jitter)
    mu, info = project_factors_to_inducing(kernel, Z, X, F, jitter=jitter, return_info=True)
    mu_w = project_factors_to_inducing(kernel, Z, X, F, jitter=jitter, whitened=True, kzz_jitter=kzz_jitter)
    assert isinstance(mu, np.ndarray) and mu.shape == mu_w.shape == info["alpha"].shape == (L, M)
    assert mu.dtype == mu_w.dtype == info["alpha"].dtype == info["residual"].dtype == F.dtype
    tol = 1e-7 if dtype == "f64" else 1e-3
    err = {}
    for what, got, want in (("mu", mu, z["mu"]), ("alpha", info["alpha"], z["alpha"]), ("mu (oracle)", mu, o["mu"].numpy()),
                            ("alpha (oracle)", info["alpha"], o["alpha"].numpy()), ("mu whitened", mu_w, o["mu_whitened"].numpy())):
        err[what] = float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())
    print(name, dtype, err, "ref32_err", float(z["ref32_err"]))
    if dtype == "f32":
        helpers.record("projection_fp32_error.jsonl", dict(case=name, observed=err, ref32_err=float(z["ref32_err"])), append=True)
    for what, e in err.items():
        assert e <= tol, (what, e)
    # the residual from G, b and alpha alone against the definition's pass over X
    rtol = 1e-9 if dtype == "f64" else 1e-4
    assert np.abs(info["residual"].astype(np.float64) - o["residual"].numpy()).max() <= 10 * rtol
    Gd = torch.diagonal(o["G"], dim1=-2, dim2=-1)
    assert info["gram_diag_min"] == pytest.approx(float(Gd.min()), rel=10 * rtol)
    assert info["gram_diag_max"] == pytest.approx(float(Gd.max()), rel=10 * rtol)


def test_scalar_kernel_shares_one_gram_matrix_bit_for_bit():
    from gpzoo import kernels as K
    from gpzoo.utilities import project_factors_to_inducing
    dat = PC.recipe(700, 130, 4, 0.5, 3, per_latent=False)
    kernel = K.RBF(float(dat["sigma"]), float(dat["lengthscale"]))
    Z, X, F = (torch.as_tensor(dat[k]).cuda() for k in ("Z", "X", "F"))
    mu, info = project_factors_to_inducing(kernel, Z, X, F, return_info=True)
    G, b = run_gram("rbf", dat, torch.float32, False, 1e-5)
    assert mu.is_cuda and mu.shape == (4, 130)
    for l in range(4):
        one, one_info = project_factors_to_inducing(kernel, Z, X, F[l:l + 1], return_info=True)
        assert torch.equal(one[0], mu[l]) and torch.equal(one_info["alpha"][0], info["alpha"][l])
        Gl, bl = run_gram("rbf", dict(dat, F=dat["F"][l:l + 1]), torch.float32, False, 1e-5)
        assert torch.equal(Gl, G) and torch.equal(bl[0, 0], b[0, l])


@pytest.mark.parametrize("kind", PO.KINDS)
def test_fp32_entries_are_the_fills_values(kind):
    """N = 1: an entry of G is one product of two generated covariance values, rounded once -- the values gpz_kfill
    writes (cov.h is the one definition of both)."""
    from gpzoo_amd import ops
    dat = PC.recipe(1, 129, 2, 1.5, 11, d=3, per_latent=True)
    spec = spec_of(kind, dat["sigma"], dat["lengthscale"], torch.float32, True)
    Z, X, F = (torch.as_tensor(dat[k]).cuda() for k in ("Z", "X", "F"))
    G, b = ops.kernel_gram(spec, Z, X, F, 0.0)
    k = ops.kfill(spec, Z, X)[:, :, 0]                                   # (L, M) fp32
    assert float(k.abs().min()) > 1e-15                                  # products stay normal numbers
    want = (k[:, :, None] * k[:, None, :]).double()
    assert torch.equal(G, want)
    assert torch.equal(b[:, 0, :], (k * F[:, :1]).double())


def test_two_calls_agree_bit_for_bit():
    from gpzoo import kernels as K
    from gpzoo.utilities import project_factors_to_inducing
    case = next(c for c in CASES if c["name"] == "far_tile_f32")
    p = PC.plan_of(case)
    assert p["n_splits"] >= 3
    dat = PC.data_of(case, p["N"])
    runs = [run_gram(case["kind"], dat, torch.float32, True, 1e-5) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    kernel = K.batched_Matern52(sigma=dat["sigma"].tolist(), lengthscale=dat["lengthscale"].tolist())
    mus = [project_factors_to_inducing(kernel, dat["Z"], dat["X"], dat["F"]) for _ in range(2)]
    np.testing.assert_array_equal(mus[0], mus[1])


@pytest.mark.parametrize("fdtype", [np.float32, np.float64])
def test_input_kinds_give_the_same_numbers(fdtype):
    from gpzoo import kernels as K
    from gpzoo.utilities import project_factors_to_inducing
    dat = PC.recipe(300, 40, 3, 0.5, 5, per_latent=True)
    kernel = K.NSF_RBF(L=3)
    kernel.sigma.data = torch.as_tensor(dat["sigma"]).reshape(3, 1, 1)
    kernel.lengthscale.data = torch.as_tensor(dat["lengthscale"]).reshape(3, 1, 1)
    Z, X, F = dat["Z"], dat["X"], dat["F"].astype(fdtype)
    a = project_factors_to_inducing(kernel, Z, X, F)
    b = project_factors_to_inducing(kernel, torch.as_tensor(Z), torch.as_tensor(X), torch.as_tensor(F))
    c = project_factors_to_inducing(kernel.cuda(), torch.as_tensor(Z).cuda(), torch.as_tensor(X).cuda(), torch.as_tensor(F).cuda())
    m = project_factors_to_inducing(kernel, torch.as_tensor(Z).cuda(), X, F)          # mixed: the output follows F
    assert isinstance(a, np.ndarray) and isinstance(m, np.ndarray) and a.dtype == fdtype
    assert isinstance(b, torch.Tensor) and not b.is_cuda and c.is_cuda and b.dtype == c.dtype == torch.as_tensor(F).dtype
    np.testing.assert_array_equal(a, b.numpy())
    np.testing.assert_array_equal(a, c.cpu().numpy())
    np.testing.assert_array_equal(a, m)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("whitened", [False, True])
def test_a_model_started_from_mu_has_the_oracles_mean(whitened, dtype):
    from gpzoo import gp as GP
    from gpzoo.utilities import project_factors_to_inducing
    name = "1037x130_L4_nsf_rbf"
    z = golden(name)
    N, M, L, frac, cls, per_latent = PC.GOLDENS[name]
    dt = tdtype(dtype)
    kernel = make_kernel(cls, z["sigma"], z["lengthscale"], L, dt).cuda()
    model = (GP.WSVGP if whitened else GP.SVGP)(kernel, dim=2, M=M, jitter=1e-4)
    Z, X, F = (torch.as_tensor(z[k]).to(dt).cuda() for k in ("Z", "X", "F"))
    model.Z.data = Z.clone()
    model.Lu.data = torch.zeros(L, M, M, dtype=dt)
    mu = project_factors_to_inducing(kernel, Z, X, F, whitened=whitened, kzz_jitter=model.jitter)
    model.mu.data = mu
    model = model.cuda()
    with torch.no_grad():
        qF = model(X)[0]
    o = PO.project("rbf", z["Z"], z["X"], z["F"], torch.as_tensor(z["sigma"]), torch.as_tensor(z["lengthscale"]),
                   jitter=1e-5, kzz_jitter=1e-4)
    want = PO.svgp_mean("rbf", z["Z"], z["X"], torch.as_tensor(z["sigma"]), torch.as_tensor(z["lengthscale"]),
                        o["mu_whitened"] if whitened else o["mu"], 1e-4, whitened)
    got = qF.mean.double().cpu()
    assert got.shape == want.shape == (L, N)
    assert float((got - want).abs().max()) <= helpers.rtol_for(dt) * float(want.abs().max())
    # and that mean is the least-squares fit of the factors: far closer to F than a zero start
    assert float(((got - torch.as_tensor(z["F"]).double()) ** 2).sum() / (torch.as_tensor(z["F"]).double() ** 2).sum()) < 0.2


def test_a_singular_gram_matrix_raises_linalgerror():
    from gpzoo import kernels as K
    from gpzoo.utilities import project_factors_to_inducing
    kernel = K.RBF(1.0, 1.0).double()
    Z, X, F = np.zeros((2, 1)), np.zeros((1, 1)), np.ones((1, 1))
    from gpzoo_amd import _lib, ops
    spec = ops.KernelSpec(_lib.KERNEL_RBF, torch.ones(1, dtype=torch.float64).cuda(), torch.ones(1, dtype=torch.float64).cuda(), False)
    G, b = ops.kernel_gram(spec, torch.as_tensor(Z).cuda(), torch.as_tensor(X).cuda(), torch.as_tensor(F).cuda(), 0.0)
    assert torch.equal(G.cpu(), torch.ones(1, 2, 2, dtype=torch.float64))          # the second pivot is exactly 0
    with pytest.raises(torch.linalg.LinAlgError):
        project_factors_to_inducing(kernel, Z, X, F, jitter=0)
    assert project_factors_to_inducing(kernel, Z, X, F, jitter=1e-5).shape == (1, 2)


def test_c_entry_refuses_before_any_launch():
    from gpzoo_amd import _lib
    from gpzoo_amd._lib import KernelDesc
    lib = _lib.load()
    t = torch.ones(64, dtype=torch.float32, device="cuda")
    G = torch.full((2, 2), -7.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())

    def gram(kind=0, d=2, R=1):
        desc = KernelDesc()
        desc.kind, desc.n_latent, desc.dtype, desc.sigma, desc.lengthscale = kind, 1, 0, t.data_ptr(), t.data_ptr()
        return lib.gpz_kernel_gram(ctypes.byref(desc), ptr(t), 2, ptr(t), 2, d, ptr(t), R, 0.0, ptr(G), ptr(G), ptr(ws), ws.numel(), None)

    for kw, msg in ((dict(kind=2), b"kind 2"), (dict(d=5), b"dimension 5"), (dict(R=65), b"R=65")):
        assert gram(**kw) < 0
        assert msg in lib.gpz_last_error()
    torch.cuda.synchronize()
    assert bool((G == -7.0).all())                                      # nothing ran
