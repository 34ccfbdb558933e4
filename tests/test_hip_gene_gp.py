"""GPU: gpz_gene_kernel_project_sparse and gpz_gene_gp_profile (csrc/gene_gp.hip) against the numpy oracle of
tests/gene_gp_cases.py on every case, with the tolerances measured there, and the bit-for-bit properties of both entries."""
import math

import numpy as np
import pytest
import torch

import gene_gp_cases as GC

pytestmark = pytest.mark.gpu
NAMES = sorted(GC.CASES)
F64 = torch.float64


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _inputs(name):
    from gpzoo_amd.likelihoods import SparseCounts
    c = GC.build_case(name)
    return c, SparseCounts(_dev(c["V"])), _dev(c["X"]), _dev(c["Z"]), _dev(c["ell"])


def _same_bits(a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.parametrize("name", NAMES)
def test_projection_against_the_oracle_and_its_bits(name):
    from gpzoo_amd import ops
    c, values, X, Z, ell = _inputs(name)
    o = GC.oracle(name)
    rtol_p, _ = GC.tolerances()
    P = ops.gene_kernel_project_sparse(values, X, Z, ell, c["kernel"])
    assert P.shape == (c["n_ell"], GC.D, c["M"]) and P.dtype == F64
    err = np.abs(P.cpu().numpy() - o["P_ref"])
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"{name}: worst |P - fsum| / sum|v k| = {np.nanmax(np.where(o['P_abs'] > 0, err / o['P_abs'], 0.0)):.3e} (RTOL_P {rtol_p:.3e})")
    assert np.all(err <= rtol_p * o["P_abs"])
    assert float(P[:, GC.EMPTY].abs().max()) == 0.0
    assert _same_bits(P, ops.gene_kernel_project_sparse(values, X, Z, ell, c["kernel"]))                 # two calls
    for wg in (1, 7):                                                                                    # the grid
        assert _same_bits(P, ops.gene_kernel_project_sparse(values, X, Z, ell, c["kernel"], workgroups=wg)), wg
    nbytes = ops.gene_kernel_project_plan(c["N"], GC.D, values.nnz, c["M"], c["n_ell"])["partials_bytes"]
    for fill in (0xFF, 0x00):                                                                            # poisoned scratch
        scratch = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
        assert _same_bits(P, ops.gene_kernel_project_sparse(values, X, Z, ell, c["kernel"], partials=scratch)), fill
    # a SparseExpression is read through its stored values
    from gpzoo_amd.likelihoods import SparseExpression
    assert _same_bits(P, ops.gene_kernel_project_sparse(SparseExpression(values, _dev(o["offset"])), X, Z, ell, c["kernel"]))


@pytest.mark.parametrize("kernel", ["rbf", "matern12", "matern32", "matern52"])
def test_one_stored_entry_gives_the_covariance_bits_of_the_gram_pass(kernel):
    """sigma = 1 and a one-hot right-hand side: gpz_kernel_gram's K_zx F^T is the covariance itself (its other terms are
    exact zeros), and so is the projection of a gene with one stored 1: the two passes generate the same K_zx."""
    from gpzoo_amd import ops
    from gpzoo_amd.likelihoods import SparseCounts
    c = GC.build_case("n257_m64_d3")
    X, Z, ell = _dev(c["X"]), _dev(c["Z"]), _dev(c["ell"])
    N, nl = c["N"], c["n_ell"]
    spots = [0, 100, N - 1]
    y = torch.zeros((len(spots), N), device="cuda")
    for g, n in enumerate(spots):
        y[g, n] = 1.0
    P = ops.gene_kernel_project_sparse(SparseCounts(y), X, Z, ell, kernel)
    spec = ops.KernelSpec(ops.GENE_GP_KINDS[kernel], torch.ones(nl, dtype=F64, device="cuda"), ell, True)
    for g, n in enumerate(spots):
        _, b = ops.kernel_gram(spec, Z, X, y[g].to(F64).expand(nl, N).contiguous(), 0.0)
        assert _same_bits(P[:, g], b[:, 0]), (kernel, n)


@pytest.mark.parametrize("name", NAMES)
def test_profile_against_the_oracle_and_its_bits(name):
    from gpzoo_amd import ops
    o = GC.oracle(name)
    c, f = o["case"], o["fit"]
    N, M = c["N"], c["M"]
    _, rtol_f = GC.tolerances()
    args = (_dev(o["p_ref"]), _dev(o["lam"]), _dev(o["yty"]), N, *c["delta_range"])
    out = ops.gene_gp_profile(*args)
    again = ops.gene_gp_profile(*args)
    for a, b in zip(out[:4], again[:4]):
        assert _same_bits(a.nan_to_num(nan=-1.0), b.nan_to_num(nan=-1.0)) and torch.equal(a.isnan(), b.isnan())
    assert torch.equal(out[4], again[4]) and torch.equal(out[5], again[5])
    F, delta, s2, tau2, status, iters = (t.cpu().numpy() for t in out)
    assert F.shape == (GC.D, c["n_ell"]) and status.dtype == np.int32 and iters.dtype == np.int32
    exempt = f["near_tied"]
    assert np.array_equal(status[~exempt], f["status"][~exempt])
    deg = f["status"] == 3
    assert np.all(status[deg] == 3) and np.all(np.isnan(F[deg])) and np.all(np.isnan(delta[deg]))
    ok = ~deg
    errF = np.abs(F[ok] - f["F"][ok]) / N
    print(f"{name}: worst |F - oracle| / N = {errF.max():.3e} (RTOL_F {rtol_f:.3e}); iterations <= {iters.max()}")
    assert np.all(errF <= rtol_f)
    cmp = ok & ~exempt
    errt = np.abs(np.log(delta[cmp]) - f["t"][cmp])
    tol = GC.delta_tolerance(name)[cmp]
    print(f"{name}: worst |t - oracle| / allowed = {(errt / tol).max():.3e}")
    assert np.all(errt <= tol)
    assert np.all(tau2[ok] == s2[ok] * delta[ok])
    # s2 is the R / N the bound was evaluated with: F rebuilt from (s2, delta) in numpy
    plan = ops.gene_gp_profile_plan(GC.D, M, c["n_ell"])
    assert iters.max() < plan["max_iter"] and np.all(iters[deg] == 0)
    lam = o["lam"][None, :, :]
    t = np.log(delta)[:, :, None]
    with np.errstate(invalid="ignore"):
        rebuilt = -0.5 * (N * math.log(2 * math.pi) + N * np.log(s2) + N + (N - M) * t[:, :, 0] + np.log(delta[:, :, None] + lam).sum(-1)
                          + (N - o["lam"].sum(-1))[None, :] / delta)
    assert np.all(np.abs(rebuilt[ok] - F[ok]) <= 1e-12 * N * np.maximum(1.0, np.abs(F[ok]) / N))
