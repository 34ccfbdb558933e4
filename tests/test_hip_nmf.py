"""GPU: the fused KL multiplicative-update NMF (gpz_nmf_kl_update, gpz_nmf_kl_divergence) against the numpy oracle, its
stopping rule and bitwise reproducibility, and regularized_nmf end to end against the reference's recorded results.
Imports only the oracle and the goldens.

Bounds.  fp64: the project's parity bar, rtol 1e-5 with atol 1e-5 max|.|.  fp32: four times delta, delta = the distance
between the REFERENCE's own float32 and float64 runs as recorded in the golden file (sklearn's BLAS sums in another
order than the MFMA tiles do, the same kind and size of error; a wrong clamp, a leaked padding lane or a stale partial
sum shows at 1e-2 or worse).  Each test prints its figures before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

import nmf_oracle as O
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES = ["nndsvdar_600x150", "nndsvda_1037x80_tol0", "nndsvd_600x150_sz", "random_600x150"]


def golden(name):
    z = np.load(os.path.join(GOLDEN, f"extra_nmf_{name}.npz"))
    return z, json.loads(str(z["kwargs"]))


def problem(N, D, L, seed=0):
    """Planted counts with an all-zero row and an all-zero column (their rows of W and columns of H go to zero at the
    first update: P < EPS is clamped from then on), and a start whose last component is zero in W and in H (den == 0 and
    ws == 0)."""
    X = O.planted_counts(N, D, L, 1000 + N + D + L + seed)
    rng = np.random.default_rng(seed + N)
    W0 = np.abs(rng.standard_normal((N, L))) + 0.05
    H0 = np.abs(rng.standard_normal((L, D))) + 0.05
    if N > 3 and D > 5:
        X[3] = 0.0
        X[:, 5] = 0.0
    if L > 2:
        W0[:, L - 1] = 0.0
        H0[L - 1] = 0.0
    return X, W0, H0


def run(X, W0, H0, iters, dtype=torch.float64):
    from gpzoo_amd import ops
    t = lambda a: torch.as_tensor(a, dtype=dtype).cuda()
    W, H, n = ops.nmf_kl_mu(t(X), t(W0), t(H0), max_iter=iters, tol=0)
    assert n == iters and W.dtype == dtype and H.dtype == dtype
    return W.double().cpu().numpy(), H.double().cpu().numpy()


def close(name, got, want, rtol, atol_rel):
    err = np.abs(got - want)
    bound = rtol * np.abs(want) + atol_rel * np.abs(want).max()
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{name}: max|err| {err.max():.3e}, max|ref| {np.abs(want).max():.3e}, worst err/bound {worst:.3e}")
    assert np.isfinite(got).all(), name
    assert (err <= bound).all(), f"{name}: worst err/bound {worst:.3e}"


SHAPES = [(1, 1, 1), (63, 17, 3), (257, 130, 5), (600, 150, 4), (1037, 80, 4), (4099, 515, 20), (3000, 400, 64),
          (130, 70, 7), (130, 70, 9), (130, 70, 13), (131, 258, 33), (130, 70, 48), (70, 1030, 2)]


@pytest.mark.parametrize("N,D,L", SHAPES)
def test_iteration_parity_fp64(N, D, L):
    X, W0, H0 = problem(N, D, L)
    W, H = W0.copy(), H0.copy()
    done = 0
    for iters in (1, 10, 200):
        for _ in range(iters - done):
            W = O.update_w(X, W, H)
            H = O.update_h(X, W, H)
        done = iters
        Wg, Hg = run(X, W0, H0, iters)
        rows = np.arange(N) if N <= 1100 else np.random.default_rng(1).choice(N, 1024, replace=False)
        close(f"W after {iters}", Wg[rows], W[rows], 1e-5, 1e-5)
        close(f"H after {iters}", Hg, H, 1e-5, 1e-5)


@pytest.mark.parametrize("case", CASES[:3])
def test_iteration_parity_fp64_from_the_golden_start(case):
    z, _ = golden(case)
    X = z["Y"].astype(np.float64)
    n = int(z["n_iter64"])
    Wg, Hg = run(X, z["W0"], z["H0"], n)
    close("W vs sklearn", Wg, z["nmfW64"], 1e-5, 1e-5)
    close("H vs sklearn", Hg, z["nmfH64"], 1e-5, 1e-5)


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("case", CASES)
def test_iteration_parity_fp32_within_four_times_the_references_own_fp32_noise(case):
    z, _ = golden(case)
    X = z["Y"].astype(np.float64)
    n = int(z["n_iter64"])
    W, H, _ = O.fit_mu(X, z["W0"], z["H0"], max_iter=n, tol=0)
    Wg, Hg = run(X, z["W0"], z["H0"], n, torch.float32)
    delta = dict(W=rel(z["nmfW32"], z["nmfW64"]), H=rel(z["nmfH32"], z["nmfH64"]),
                 WH=rel(z["nmfW32"].astype(np.float64) @ z["nmfH32"], z["nmfW64"] @ z["nmfH64"]))
    got = dict(W=rel(Wg, W), H=rel(Hg, H), WH=rel(Wg @ Hg, W @ H))
    for k in ("W", "H", "WH"):
        print(f"{case} {k}: kernel fp32 vs fp64 oracle {got[k]:.3e}, reference's delta {delta[k]:.3e}, bound {4 * delta[k]:.3e}")
    for k in ("W", "H", "WH"):
        assert got[k] <= 4 * delta[k], (k, got[k], delta[k])


@pytest.mark.parametrize("N,D,L", [(63, 17, 3), (600, 150, 4), (4099, 515, 20), (3000, 400, 64), (70001, 130, 5)])
def test_divergence(N, D, L):
    from gpzoo_amd import ops
    X, W0, H0 = problem(N, D, L, seed=3)
    for dtype, rtol in ((torch.float64, 1e-10), (torch.float32, 1e-5)):
        t = [torch.as_tensor(a, dtype=dtype).cuda() for a in (X, W0, H0)]
        got = ops.nmf_kl_divergence(*t)
        want = O.kl_divergence(*[a.double().cpu().numpy() for a in t])
        print(f"{dtype}: {got!r} vs {want!r}, rel {abs(got - want) / want:.3e}")
        assert abs(got - want) <= rtol * want
        assert ops.nmf_kl_divergence(*t) == got


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_stopping_rule_stops_where_sklearn_stops(case, dtype):
    from gpzoo_amd import ops
    z, kw = golden(case)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=dtype).cuda()
    W0, H0 = t(z["W0"]), t(z["H0"])
    keep = W0.clone(), H0.clone()
    _, _, n = ops.nmf_kl_mu(t(z["Y"]), W0, H0, max_iter=kw["max_iter"], tol=kw.get("tol", 1e-4))
    print(f"{case} {dtype}: n_iter {n}, golden {int(z['n_iter64'])} / {int(z['n_iter32'])}")
    assert n == int(z["n_iter64"]) == int(z["n_iter32"])
    assert torch.equal(W0, keep[0]) and torch.equal(H0, keep[1])          # the starting values are copied


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_bitwise_reproducible_and_splittable(dtype):
    from gpzoo_amd import ops
    X, W0, H0 = problem(70001, 130, 5)                       # several slabs
    t = [torch.as_tensor(a, dtype=dtype).cuda() for a in (X, W0, H0)]
    Wa, Ha, _ = ops.nmf_kl_mu(*t, max_iter=20, tol=0)
    Wb, Hb, _ = ops.nmf_kl_mu(*t, max_iter=20, tol=0)
    assert torch.equal(Wa, Wb) and torch.equal(Ha, Hb)
    W1, H1, _ = ops.nmf_kl_mu(*t, max_iter=10, tol=0)
    W2, H2, _ = ops.nmf_kl_mu(t[0], W1, H1, max_iter=10, tol=0)
    assert torch.equal(Wa, W2) and torch.equal(Ha, H2)
    assert torch.isfinite(Wa).all() and torch.isfinite(Ha).all()


def end_to_end(z, kw, Y):
    from gpzoo.utilities import regularized_nmf
    sz = z["sz"] if z["sz"].ndim else 1
    return regularized_nmf(Y, int(z["L"]), sz=sz, shrinkage=float(z["shrinkage"]), **kw)


@pytest.mark.parametrize("case", CASES)
def test_regularized_nmf_fp64_against_the_reference(case):
    z, kw = golden(case)
    Y = z["Y"].astype(np.float64)
    F, W = end_to_end(z, kw, Y)
    assert isinstance(F, np.ndarray) and isinstance(W, np.ndarray)
    assert (F.dtype, W.dtype, F.shape, W.shape) == (z["F64"].dtype, z["W64"].dtype, z["F64"].shape, z["W64"].shape)
    close("F", F, z["F64"], 1e-5, 1e-5)
    close("W", W, z["W64"], 1e-5, 1e-5)
    for other in (torch.as_tensor(Y), torch.as_tensor(Y).cuda()):      # a CPU tensor and a CUDA tensor give the same bits
        F2, W2 = end_to_end(z, kw, other)
        np.testing.assert_array_equal(F2, F)
        np.testing.assert_array_equal(W2, W)


@pytest.mark.parametrize("case", CASES)
def test_regularized_nmf_fp32_within_four_times_the_references_own_fp32_noise(case):
    z, kw = golden(case)
    Y = z["Y"].astype(np.float32)
    F, W = end_to_end(z, kw, Y)
    assert (F.dtype, W.dtype, F.shape, W.shape) == (z["F32"].dtype, z["W32"].dtype, z["F32"].shape, z["W32"].shape)
    dF, dW = np.abs(z["F32"] - z["F64"]).max(), np.abs(z["W32"] - z["W64"]).max()
    eF, eW = np.abs(F - z["F64"]).max(), np.abs(W - z["W64"]).max()
    print(f"{case}: F err {eF:.3e} (delta {dF:.3e}), W err {eW:.3e} (delta {dW:.3e})")
    assert np.isfinite(F).all() and np.isfinite(W).all()
    assert eF <= 4 * dF and eW <= 4 * dW
    F2, W2 = end_to_end(z, kw, torch.as_tensor(Y).cuda())
    np.testing.assert_array_equal(F2, F)
    np.testing.assert_array_equal(W2, W)


def test_regularized_nmf_input_errors():
    from gpzoo.utilities import regularized_nmf
    kw = dict(solver="mu", beta_loss="kullback-leibler", init="nndsvd", max_iter=5)
    Y = O.planted_counts(40, 12, 3, 0)
    for bad in (-1.0, np.nan, np.inf):
        Yb = Y.copy()
        Yb[7, 3] = bad
        with pytest.raises(ValueError, match="negative or non-finite"):
            regularized_nmf(Yb, 3, **kw)
    with pytest.raises(ValueError, match="min"):
        regularized_nmf(Y, 13, **kw)
    with pytest.raises(ValueError, match="L=65"):
        regularized_nmf(Y, 65, **dict(kw, init="random"))
    with pytest.raises(ValueError, match="L=0"):
        regularized_nmf(Y, 0, **kw)
    with pytest.raises(ValueError, match="2-D|obs, feat"):
        regularized_nmf(Y[0], 3, **kw)
    with pytest.raises(ValueError, match="size factors"):
        regularized_nmf(Y, 3, sz=np.ones((39, 1)), **kw)
    F, W = regularized_nmf(Y, 3, sz=np.ones((40, 1)), **kw)
    assert F.shape == (40, 3) and W.shape == (12, 3)


def test_ops_reject_mismatched_arguments():
    from gpzoo_amd import ops
    X = torch.ones(8, 5, dtype=torch.float64).cuda()
    with pytest.raises(ValueError, match="expected"):
        ops.nmf_kl_mu(X, torch.ones(8, 2).double().cuda(), torch.ones(3, 5).double().cuda())
    with pytest.raises(TypeError, match="dtype"):
        ops.nmf_kl_mu(X, torch.ones(8, 2).cuda(), torch.ones(2, 5).cuda())
    with pytest.raises(ValueError, match="L=65"):
        ops.nmf_kl_divergence(X, torch.ones(8, 65).double().cuda(), torch.ones(65, 5).double().cuda())
