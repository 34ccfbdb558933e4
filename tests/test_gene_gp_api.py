"""utilities.gene_spatial_gp and rank_genes(by="gp"): the refusals, the plan queries and the C ABI's argument errors on the
CPU (nothing is launched); the assembly end to end against the numpy oracle of tests/gene_gp_cases.py on the GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import gene_gp_cases as GC
from conftest import ROOT

SYMBOLS = ("gpz_gene_kernel_project_sparse", "gpz_gene_kernel_project_sparse_plan", "gpz_gene_gp_profile", "gpz_gene_gp_profile_plan")
FIELDS = ("lengthscale", "ell_index", "loglik", "null_loglik", "lr", "pvalue", "s2", "tau2", "delta", "fsv", "status", "loglik_grid",
          "lengthscales", "Z")


def test_symbols_sources_and_flags():
    from gpzoo_amd import _lib, build, ops
    hdr = open(os.path.join(ROOT, "include", "gpzoo_hip.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert f"{name}(" in hdr and name in _lib.exported_symbols() and hasattr(lib, name)
    assert "gene_gp.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "gene_gp.hip"))
    assert "-ffp-contract=off" in build.SOURCE_FLAGS["gene_gp.hip"]
    assert lib.gpz_version() == 212
    assert all(callable(getattr(ops, n)) for n in ("gene_kernel_project_sparse", "gene_kernel_project_plan", "gene_gp_profile",
                                                   "gene_gp_profile_plan"))
    src = open(os.path.join(build.CSRC, "gene_gp.hip")).read()
    assert not re.search(r"\batomic(Add|Max|Min|Exch|CAS)", src)                 # fixed-order sums, no atomics on values


def test_plan_queries():
    from gpzoo_amd import ops
    p = ops.gene_kernel_project_plan(39694, 17702, 35_000_000, 256, 8)
    assert p["gene_chunk"] % 256 == 0 and 4 * p["gene_chunk"] >= 39694 > 3 * p["gene_chunk"]
    assert p["partials_bytes"] < 39694 * 256 * 8                                   # less than one stored K_xz
    assert not p["generate"] and ops.gene_kernel_project_plan(39694, 17702, 7_000_000, 256, 8)["generate"]
    assert ops.gene_kernel_project_plan(1000, 48, 290 * 1000, 64, 4)["generate"]
    assert not ops.gene_kernel_project_plan(1000, 48, 290 * 1000 + 1, 64, 4)["generate"]
    assert ops.gene_kernel_project_plan(65, 48, 100, 8, 1)["gene_chunk"] == 256
    assert ops.gene_kernel_project_plan(1037, 48, 100, 8, 1)["gene_chunk"] == 512
    q = ops.gene_gp_profile_plan(48, 129, 9)
    assert q["grid_points"] == 33 and 0 < q["tol_t"] <= 1e-8 and q["max_iter"] >= 50 and q["workgroups"] == 48 * 9
    for bad in ((100, 48, 10, 0, 4), (100, 48, 10, 1025, 4), (100, 48, 10, 64, 17), (100, 48, 10, 64, 0), (0, 48, 10, 64, 4)):
        with pytest.raises(ValueError, match="gpz_gene_kernel_project_sparse"):
            ops.gene_kernel_project_plan(*bad)
    for bad in ((48, 0, 4), (48, 1025, 4), (48, 64, 17), (0, 64, 4)):
        with pytest.raises(ValueError, match="gpz_gene_gp_profile"):
            ops.gene_gp_profile_plan(*bad)


def test_argument_errors_come_back_as_codes_with_messages():
    """Every check runs on the host before any launch: the pointers are never read."""
    from gpzoo_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)

    def project(N=100, D=4, nnz=10, M=8, d=2, nl=4, kind=0, wg=0, nbytes=1 << 30, partials=ptr):
        return lib.gpz_gene_kernel_project_sparse(*([ptr] * 7), N, D, nnz, M, d, nl, kind, wg, ptr, partials, nbytes, None)

    for kw, msg in ((dict(M=0), b"M = 0"), (dict(M=1025), b"M = 1025"), (dict(nl=17), b"n_ell = 17"), (dict(nl=0), b"n_ell = 0"),
                    (dict(d=5), b"dimension 5"), (dict(d=0), b"dimension 0"), (dict(kind=2), b"kind 2"), (dict(N=0), b"extents"),
                    (dict(wg=-1), b"workgroups"), (dict(nbytes=8), b"partials too small"), (dict(partials=None), b"null pointer")):
        assert project(**kw) == -1, kw
        err = lib.gpz_last_error()
        assert msg in err and b"gpz_gene_kernel_project_sparse" in err, (kw, err)

    def profile(N=100, D=4, M=8, nl=4, lo=1e-3, hi=1e6, p=ptr):
        return lib.gpz_gene_gp_profile(p, ptr, ptr, N, D, M, nl, lo, hi, *([ptr] * 6), None)

    for kw, msg in ((dict(M=0), b"M = 0"), (dict(M=1025), b"M = 1025"), (dict(nl=17), b"n_ell = 17"), (dict(N=1), b"N = 1"),
                    (dict(lo=0.0), b"delta range"), (dict(lo=2.0, hi=1.0), b"delta range"), (dict(p=None), b"null pointer")):
        assert profile(**kw) == -1, kw
        err = lib.gpz_last_error()
        assert msg in err and b"gpz_gene_gp_profile" in err, (kw, err)


def test_refusals_before_any_device_work():
    from gpzoo_amd import ops
    from gpzoo_amd.likelihoods import SparseCounts, SparseExpression
    import gpzoo.utilities as ut
    assert ut.gene_spatial_gp is not None and ut.GeneSpatialGP._fields == FIELDS
    counts = SparseCounts(torch.tensor([[0., 2., 1., 0.], [3., 0., 0., 1.]]))
    expr = ut.log_normalize(counts)
    X = torch.rand(4, 2, dtype=torch.float64)
    with pytest.raises(TypeError, match="log_normalize"):
        ut.gene_spatial_gp(counts, X)
    with pytest.raises(TypeError, match="view"):
        ut.gene_spatial_gp(expr[:, torch.tensor([0, 1])], X)
    with pytest.raises(TypeError, match=r"\.T"):
        ut.gene_spatial_gp(counts.T, X)
    with pytest.raises(TypeError):
        ut.gene_spatial_gp([[1.0, 2.0]], X)
    with pytest.raises(ValueError, match="coords"):
        ut.gene_spatial_gp(expr, torch.rand(5, 2))
    with pytest.raises(ValueError, match="kernel"):
        ut.gene_spatial_gp(expr, X, kernel="periodic")
    with pytest.raises(ValueError, match="delta_range"):
        ut.gene_spatial_gp(expr, X, delta_range=(1.0, 0.5))
    with pytest.raises(ValueError, match="inducing"):
        ut.gene_spatial_gp(expr, X, inducing=5)
    with pytest.raises(TypeError, match="view"):
        ops.gene_kernel_project_sparse(counts[:, torch.tensor([0, 1])], X, X, torch.ones(1, dtype=torch.float64))
    with pytest.raises(ValueError, match="coords"):
        ut.rank_genes(counts, by="gp")
    assert SparseExpression is not None


def _api_inputs():
    from gpzoo_amd.likelihoods import SparseCounts, SparseExpression
    o = GC.oracle(GC.API_CASE)
    c = o["case"]
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    expr = SparseExpression(SparseCounts(dev(c["V"])), dev(o["offset"]))
    return o, c, expr, dev(c["X"]), dev(c["Z"]), dev(c["ell"])


@pytest.mark.gpu
def test_end_to_end_against_the_oracle():
    import gpzoo.utilities as ut
    o, c, expr, X, Z, ell = _api_inputs()
    f, N, nl = o["fit"], c["N"], c["n_ell"]
    r = ut.gene_spatial_gp(expr, X, inducing=Z, kernel=c["kernel"], lengthscales=ell, delta_range=c["delta_range"], jitter=GC.JITTER)
    shapes = dict(loglik_grid=(GC.D, nl), lengthscales=(nl,), Z=tuple(Z.shape))
    for name in FIELDS:
        t = getattr(r, name)
        assert tuple(t.shape) == shapes.get(name, (GC.D,)), name
        assert t.dtype == {"ell_index": torch.int64, "status": torch.int32}.get(name, torch.float64), name
        assert t.is_cuda
    # The device factors K_zz + jitter I and diagonalises Phi Phi^T on its own: Phi differs from the oracle's by the backward
    # error of a Cholesky factorisation and two triangular solves, a few eps times cond(K_zz + jitter I) in relative terms,
    # and the bound is a sum over N spots of terms whose sensitivity to a relative change of Phi is of order one.
    _, rtol_f = GC.tolerances()
    tol = N * (rtol_f + 8 * np.finfo(np.float64).eps * o["cond"].max())
    deg = f["status"][:, 0] == 3
    grid = r.loglik_grid.cpu().numpy()
    err = np.abs(grid[~deg] - f["F"][~deg])
    print(f"end to end: worst |F - oracle| = {err.max():.3e} (allowed {tol:.3e})")
    assert np.all(err <= tol) and np.all(np.isnan(grid[deg]))
    status = r.status.cpu().numpy()
    assert np.all(status[deg] == 3) and np.all(np.isnan(r.lr.cpu().numpy()[deg]))
    srt = np.sort(f["F"][~deg], axis=1)
    clear = np.flatnonzero(~deg)[(nl == 1) | (srt[:, -1] - srt[:, -2] > 2 * tol)]       # the best length scale is not a near tie
    best = o["best"]
    assert np.array_equal(r.ell_index.cpu().numpy()[clear], best[clear])
    assert np.array_equal(r.lengthscale.cpu().numpy()[clear], c["ell"][best[clear]])
    pick = lambda a: a[clear, best[clear]]
    assert np.array_equal(status[clear], pick(f["status"]))
    lr = np.maximum(2.0 * (pick(f["F"]) - o["null"][clear]), 0.0)
    assert np.all(np.abs(r.lr.cpu().numpy()[clear] - lr) <= 2 * tol + 1e-12 * np.abs(o["null"][clear]))
    assert np.all(np.abs(r.null_loglik.cpu().numpy()[clear] - o["null"][clear]) <= 1e-12 * np.abs(o["null"][clear]))
    got_lr = r.lr.cpu().numpy()[clear]
    assert np.allclose(r.pvalue.cpu().numpy()[clear], [math.erfc(math.sqrt(v / 2)) for v in got_lr], rtol=1e-12, atol=0)
    # delta, and with it fsv = gamma / (gamma + delta), move by the shift in t the tolerance on F allows at the optimum
    with np.errstate(invalid="ignore", divide="ignore"):
        shift = GC.delta_tolerance(GC.API_CASE)[clear, best[clear]] + np.sqrt(tol / np.abs(pick(f["curvature"])))
    interior = pick(f["status"]) == 0
    dt = np.abs(np.log(r.delta.cpu().numpy()[clear]) - pick(f["t"]))
    assert np.all(dt[interior] <= shift[interior]) and np.all(dt[~interior] <= 1e-12)
    gamma = o["gamma"][best[clear]]
    want = gamma / (gamma + np.exp(pick(f["t"])))
    assert np.all(np.abs(r.fsv.cpu().numpy()[clear] - want) <= 0.25 * np.where(interior, shift, 0.0) + 1e-9)
    planted = [g for g in GC.PLANTED]
    assert r.lr[planted].min() > r.lr[list(GC.NOISE)].max()


@pytest.mark.gpu
def test_the_gathered_projection_agrees_with_the_generated_one():
    """The path gene_spatial_gp takes above the plan's density: a stored K_xz per length scale, gathered.  Its covariances
    may differ from the generated ones in the last bits and its sums run in another order: either sum is within
    (n + 2) eps sum|v k| of the exact one for n stored entries, the two within twice that."""
    from gpzoo_amd import ops
    o, c, expr, X, Z, ell = _api_inputs()
    a = ops.gene_kernel_project_sparse(expr, X, Z, ell, c["kernel"]).cpu().numpy()
    b = ops.gene_kernel_project_gather(expr, X, Z, ell, c["kernel"]).cpu().numpy()
    n = (c["V"] != 0).sum(axis=1)[None, :, None]
    assert np.all(np.abs(a - b) <= 2 * (n + 2) * np.finfo(np.float64).eps * o["P_abs"])


@pytest.mark.gpu
def test_dense_input_gives_the_bits_of_the_equal_sparse_expression():
    import gpzoo.utilities as ut
    from gpzoo_amd.likelihoods import SparseCounts, SparseExpression, _gene_moments
    o, c, _, X, Z, ell = _api_inputs()
    dense = torch.as_tensor(c["V"]).cuda()
    stored = SparseCounts(dense)
    zero = torch.zeros(GC.D, dtype=torch.float64, device="cuda")
    expr = SparseExpression(stored, _gene_moments(SparseExpression(stored, zero))[0] / c["N"])
    kw = dict(inducing=Z, kernel=c["kernel"], lengthscales=ell)
    a, b = ut.gene_spatial_gp(dense, X, **kw), ut.gene_spatial_gp(expr, X, **kw)
    for name in FIELDS:
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x.isnan(), y.isnan()) and torch.equal(x.nan_to_num(nan=0.0), y.nan_to_num(nan=0.0)), name


@pytest.mark.gpu
def test_inducing_as_an_int_and_the_default_length_scales():
    import gpzoo.utilities as ut
    o, c, expr, X, _, _ = _api_inputs()
    r = ut.gene_spatial_gp(expr, X, inducing=40, seed=3)
    assert tuple(r.Z.shape) == (40, c["d"]) and torch.unique(r.Z, dim=0).shape[0] == 40
    assert r.lengthscales.numel() == 8 and bool((r.lengthscales[1:] > r.lengthscales[:-1]).all())
    side = X.max(dim=0).values - X.min(dim=0).values
    assert abs(float(r.lengthscales[-1]) - 0.5 * float(side.max())) < 1e-12
    assert abs(float(r.lengthscales[0]) - float(side.prod() / 40) ** (1.0 / c["d"])) < 1e-12
    live = r.status != 3
    assert int(live.sum()) == GC.D - 2
    for name in ("loglik", "null_loglik", "lr", "pvalue", "s2", "tau2", "delta", "fsv"):
        assert bool(torch.isfinite(getattr(r, name)[live]).all()), name
    assert bool((r.lr[live] >= 0).all() & (r.pvalue[live] >= 0).all() & (r.pvalue[live] <= 1).all())
    assert bool((r.fsv[live] >= 0).all() & (r.fsv[live] <= 1).all())
    again = ut.gene_spatial_gp(expr, X, inducing=40, seed=3)
    assert torch.equal(r.loglik_grid.nan_to_num(nan=0.0), again.loglik_grid.nan_to_num(nan=0.0))


@pytest.mark.gpu
def test_rank_genes_by_gp_puts_planted_genes_first():
    import gpzoo.utilities as ut
    from gpzoo_amd.likelihoods import SparseCounts
    o, c, _, X, Z, ell = _api_inputs()
    genes = list(GC.NOISE) + list(GC.PLANTED)
    counts = SparseCounts(torch.as_tensor(np.rint(np.expm1(c["V"][genes].astype(np.float64))).astype(np.float32)).cuda())
    # unit size factors: the scored values are then the case's own log1p counts (the spot totals of these few genes carry the
    # planted structure, and dividing by them would plant it in the noise genes)
    kw = dict(coords=X, size_factors=np.ones(c["N"]), inducing=Z, kernel=c["kernel"], lengthscales=ell)
    order, score = ut.rank_genes(counts, by="gp", **kw)
    assert order.dtype == torch.int64 and tuple(order.shape) == (len(genes),) and bool((score[:-1] >= score[1:]).all())
    n_noise = len(GC.NOISE)
    assert set(order[:len(GC.PLANTED)].tolist()) == set(range(n_noise, len(genes)))
    top, _ = ut.rank_genes(counts, by="gp", nfeat=5, **kw)
    assert torch.equal(top, order[:5])
