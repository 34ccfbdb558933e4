"""GPU: the KL multiplicative-update NMF over the stored non-zeros of a SparseCounts (gpz_nmf_kl_sparse_update,
gpz_nmf_kl_sparse_divergence, gpz_counts_matmul) against the numpy oracle on the dense array of the same case, its stopping
rule and bitwise reproducibility, regularized_nmf(counts.T) end to end against the reference's recorded results, and the
initialisation chain example on sparse counts.  Imports only the oracle, the case builders and the goldens.

Bounds are those of tests/test_hip_nmf.py.  fp64: the project's parity bar, rtol 1e-5 with atol 1e-5 max|.|; one dropped or
doubled non-zero out of the ~1e3 of the longest row moves its factor row by about 1e-3 after one iteration.  fp32: four
times delta, delta = the distance between the REFERENCE's own float32 and float64 runs as recorded in the golden file (a
different summation order is the same kind and size of error).  Each test prints its figures before it asserts."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import nmf_oracle as O
import sparse_nmf_cases as SC
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

CASES = ["nndsvdar_600x150", "nndsvda_1037x80_tol0", "nndsvd_600x150_sz", "random_600x150"]


def golden(name):
    z = np.load(os.path.join(GOLDEN, f"extra_nmf_{name}.npz"))
    return z, json.loads(str(z["kwargs"]))


def cuda_counts(X):
    return SC.counts_of(X).cuda()


def run(counts, W0, H0, iters, dtype=torch.float64):
    from gpzoo_amd import ops
    t = lambda a: torch.as_tensor(a, dtype=dtype).cuda()
    W, H, n = ops.nmf_kl_mu_sparse(counts, t(W0), t(H0), max_iter=iters, tol=0)
    assert n == iters and W.dtype == dtype and H.dtype == dtype
    return W.double().cpu().numpy(), H.double().cpu().numpy()


def close(name, got, want, rtol, atol_rel):
    err = np.abs(got - want)
    bound = rtol * np.abs(want) + atol_rel * np.abs(want).max()
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{name}: max|err| {err.max():.3e}, max|ref| {np.abs(want).max():.3e}, worst err/bound {worst:.3e}")
    assert np.isfinite(got).all(), name
    assert (err <= bound).all(), f"{name}: worst err/bound {worst:.3e}"


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("name", SC.names())
def test_iteration_parity_fp64(name):
    case = SC.named(name)
    counts = cuda_counts(case["X"])
    ref = SC.oracle_iterates(name)
    print(f"{name}: X {case['X'].shape}, L {case['W0'].shape[1]}, nnz {counts.nnz}")
    for iters, (W, H) in ref.items():
        Wg, Hg = run(counts, case["W0"], case["H0"], iters)
        close(f"W after {iters}", Wg, W, 1e-5, 1e-5)
        close(f"H after {iters}", Hg, H, 1e-5, 1e-5)
        if name == "all_zero":
            assert not Wg.any() and not Hg.any()


def test_all_zero_matrix_goes_to_zero_and_its_divergence_is_the_oracles():
    from gpzoo_amd import ops
    case = SC.named("all_zero")
    counts = cuda_counts(case["X"])
    assert counts.nnz == 0
    for dtype in (torch.float64, torch.float32):
        W0, H0 = (torch.as_tensor(case[k], dtype=dtype).cuda() for k in ("W0", "H0"))
        W, H, _ = ops.nmf_kl_mu_sparse(counts, W0, H0, max_iter=1, tol=0)
        assert torch.isfinite(W).all() and torch.isfinite(H).all() and not W.any() and not H.any()
        got = ops.nmf_kl_divergence_sparse(counts, W0, H0)
        want = O.kl_divergence(case["X"], W0.double().cpu().numpy(), H0.double().cpu().numpy())
        print(f"{dtype}: divergence {got!r} vs {want!r}")
        assert abs(got - want) <= 1e-10 * want
        assert ops.nmf_kl_divergence_sparse(counts, W, H) == 0.0


@pytest.mark.parametrize("case", CASES)
def test_iteration_parity_fp32_within_four_times_the_references_own_fp32_noise(case):
    z, _ = golden(case)
    X = z["Y"].astype(np.float64)
    n = int(z["n_iter64"])
    W, H, _ = O.fit_mu(X, z["W0"], z["H0"], max_iter=n, tol=0)
    Wg, Hg = run(cuda_counts(X), z["W0"], z["H0"], n, torch.float32)
    delta = dict(W=rel(z["nmfW32"], z["nmfW64"]), H=rel(z["nmfH32"], z["nmfH64"]),
                 WH=rel(z["nmfW32"].astype(np.float64) @ z["nmfH32"], z["nmfW64"] @ z["nmfH64"]))
    got = dict(W=rel(Wg, W), H=rel(Hg, H), WH=rel(Wg @ Hg, W @ H))
    for k in ("W", "H", "WH"):
        print(f"{case} {k}: kernel fp32 vs fp64 oracle {got[k]:.3e}, reference's delta {delta[k]:.3e}, bound {4 * delta[k]:.3e}")
    for k in ("W", "H", "WH"):
        assert got[k] <= 4 * delta[k], (k, got[k], delta[k])


@pytest.mark.parametrize("name", ["small", "chunked", "all_zero"])
def test_divergence(name):
    from gpzoo_amd import ops
    case = SC.named(name)
    counts = cuda_counts(case["X"])
    for dtype, rtol in ((torch.float64, 1e-10), (torch.float32, 1e-5)):
        W, H = (torch.as_tensor(case[k], dtype=dtype).cuda() for k in ("W0", "H0"))
        got = ops.nmf_kl_divergence_sparse(counts, W, H)
        want = O.kl_divergence(case["X"], W.double().cpu().numpy(), H.double().cpu().numpy())
        print(f"{name} {dtype}: {got!r} vs {want!r}, rel {abs(got - want) / want:.3e}")
        assert abs(got - want) <= rtol * want
        assert ops.nmf_kl_divergence_sparse(counts, W, H) == got
        assert ops.nmf_kl_divergence_sparse(counts.T, W, H) == got           # the counts or their .T


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_stopping_rule_stops_where_sklearn_stops(case, dtype):
    from gpzoo_amd import ops
    z, kw = golden(case)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=dtype).cuda()
    W0, H0 = t(z["W0"]), t(z["H0"])
    keep = W0.clone(), H0.clone()
    _, _, n = ops.nmf_kl_mu_sparse(cuda_counts(z["Y"]).T, W0, H0, max_iter=kw["max_iter"], tol=kw.get("tol", 1e-4))
    print(f"{case} {dtype}: n_iter {n}, golden {int(z['n_iter64'])} / {int(z['n_iter32'])}")
    assert n == int(z["n_iter64"]) == int(z["n_iter32"])
    assert torch.equal(W0, keep[0]) and torch.equal(H0, keep[1])          # the starting values are copied


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_bitwise_reproducible_and_splittable(dtype):
    from gpzoo_amd import ops
    case = SC.named("chunked")
    counts = cuda_counts(case["X"])
    W0, H0 = (torch.as_tensor(case[k], dtype=dtype).cuda() for k in ("W0", "H0"))
    Wa, Ha, _ = ops.nmf_kl_mu_sparse(counts, W0, H0, max_iter=20, tol=0)
    Wb, Hb, _ = ops.nmf_kl_mu_sparse(counts, W0, H0, max_iter=20, tol=0)
    assert torch.equal(Wa, Wb) and torch.equal(Ha, Hb)
    W1, H1, _ = ops.nmf_kl_mu_sparse(counts, W0, H0, max_iter=10, tol=0)
    W2, H2, _ = ops.nmf_kl_mu_sparse(counts, W1, H1, max_iter=10, tol=0)
    assert torch.equal(Wa, W2) and torch.equal(Ha, H2)
    assert torch.isfinite(Wa).all() and torch.isfinite(Ha).all() and Wa.any() and Ha.any()


@pytest.mark.parametrize("k", [1, 11, 74])
def test_counts_matmul_both_orientations(k):
    from gpzoo_amd import ops
    X = SC.named("chunked")["X"]
    counts = cuda_counts(X)
    rng = np.random.default_rng(k)
    for transpose in (False, True):
        Q = rng.standard_normal((X.shape[0] if transpose else X.shape[1], k))
        want = (X.T if transpose else X) @ Q
        Qd = torch.as_tensor(Q).cuda()
        got = ops.counts_matmul(counts.T if transpose else counts, Qd, transpose=transpose)
        assert got.dtype == torch.float64 and tuple(got.shape) == want.shape
        err = np.abs(got.cpu().numpy() - want).max()
        print(f"k {k} transpose {transpose}: max|err| {err:.3e}, max|ref| {np.abs(want).max():.3e}")
        assert err <= 1e-12 * np.abs(want).max()
        assert torch.equal(ops.counts_matmul(counts, Qd, transpose=transpose), got)


def end_to_end(z, kw, Y):
    from gpzoo.utilities import regularized_nmf
    sz = z["sz"] if z["sz"].ndim else 1
    return regularized_nmf(Y, int(z["L"]), sz=sz, shrinkage=float(z["shrinkage"]), **kw)


@pytest.mark.parametrize("case", CASES)
def test_regularized_nmf_fp64_against_the_reference(case):
    z, kw = golden(case)
    cpu = SC.counts_of(z["Y"])
    F, W = end_to_end(z, kw, cpu.T.double())
    assert isinstance(F, np.ndarray) and isinstance(W, np.ndarray)
    assert (F.dtype, W.dtype, F.shape, W.shape) == (z["F64"].dtype, z["W64"].dtype, z["F64"].shape, z["W64"].shape)
    close("F", F, z["F64"], 1e-5, 1e-5)
    close("W", W, z["W64"], 1e-5, 1e-5)
    F2, W2 = end_to_end(z, kw, cpu.cuda().T.double())                  # CPU-resident and CUDA-resident counts: the same bits
    np.testing.assert_array_equal(F2, F)
    np.testing.assert_array_equal(W2, W)


@pytest.mark.parametrize("case", CASES)
def test_regularized_nmf_fp32_within_four_times_the_references_own_fp32_noise(case):
    z, kw = golden(case)
    cpu = SC.counts_of(z["Y"])
    F, W = end_to_end(z, kw, cpu.T)
    assert (F.dtype, W.dtype, F.shape, W.shape) == (z["F32"].dtype, z["W32"].dtype, z["F32"].shape, z["W32"].shape)
    dF, dW = np.abs(z["F32"] - z["F64"]).max(), np.abs(z["W32"] - z["W64"]).max()
    eF, eW = np.abs(F - z["F64"]).max(), np.abs(W - z["W64"]).max()
    print(f"{case}: F err {eF:.3e} (delta {dF:.3e}), W err {eW:.3e} (delta {dW:.3e})")
    assert np.isfinite(F).all() and np.isfinite(W).all()
    assert eF <= 4 * dF and eW <= 4 * dW
    F2, W2 = end_to_end(z, kw, cpu.cuda().T.float())
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
            regularized_nmf(SC.counts_of(Yb).T, 3, **kw)
    counts = SC.counts_of(Y)
    with pytest.raises(ValueError, match="min"):
        regularized_nmf(counts.T, 13, **kw)
    with pytest.raises(ValueError, match="L=65"):
        regularized_nmf(counts.T, 65, **dict(kw, init="random"))
    with pytest.raises(ValueError, match="L=0"):
        regularized_nmf(counts.T, 0, **kw)
    with pytest.raises(ValueError, match="size factors"):
        regularized_nmf(counts.T, 3, sz=np.ones((39, 1)), **kw)
    F, W = regularized_nmf(counts.T, 3, sz=np.ones((40, 1)), **kw)
    assert F.shape == (40, 3) and W.shape == (12, 3)


def test_ops_reject_mismatched_arguments():
    from gpzoo_amd import ops
    counts = cuda_counts(SC.named("small")["X"])                          # (17 genes, 63 spots)
    with pytest.raises(ValueError, match="expected"):
        ops.nmf_kl_mu_sparse(counts, torch.ones(63, 2).double().cuda(), torch.ones(3, 17).double().cuda())
    with pytest.raises(TypeError, match="dtype"):
        ops.nmf_kl_mu_sparse(counts, torch.ones(63, 2).cuda(), torch.ones(2, 17).double().cuda())
    with pytest.raises(ValueError, match="L=65"):
        ops.nmf_kl_divergence_sparse(counts, torch.ones(63, 65).double().cuda(), torch.ones(65, 17).double().cuda())
    with pytest.raises(RuntimeError, match="counts live on"):
        ops.nmf_kl_mu_sparse(counts.cpu(), torch.ones(63, 2).cuda(), torch.ones(2, 17).cuda())
    with pytest.raises(ValueError, match="k=129"):
        ops.counts_matmul(counts, torch.ones(17, 129).double().cuda())


def test_init_chain_example_runs_on_sparse_counts():
    cmd = [sys.executable, os.path.join(ROOT, "examples", "nsf_init_chain.py"), "--sparse-counts", "0.05", "--spots", "2000",
           "--genes", "100", "--inducing", "100", "--steps", "3"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0
    assert "sparse counts:" in p.stdout
    losses = re.findall(r"loss (\S+) -> (\S+)", p.stdout)
    assert len(losses) == 2
    for first, last in losses:
        assert np.isfinite(float(first)) and float(last) < float(first), (first, last)
