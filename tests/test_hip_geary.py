"""GPU: Geary's C, the kurtosis and the permutation null of C (gpzoo_amd/csrc/spatial_stats.hip, moran_expr.h, the Geary
instantiations of moran_perm.hip) against the oracles and within the recorded bounds of tests/geary_cases.py; I with the bits
of the Moran-only entries; every output with the same bits whatever the batch, the line's home and the scratch memory's
contents; the mean and variance over all 7! relabellings against the analytic randomisation moments."""
import functools

import numpy as np
import pytest
import torch

import gene_rank_cases as G
import geary_cases as Y
import moran_perm_cases as M

pytestmark = pytest.mark.gpu

FIELDS = ("value", "n_ge", "n_le", "sim_mean", "sim_m2", "sims")
MORAN_FIELDS = ("I",) + FIELDS[1:]
DENSE_K = 6


@functools.lru_cache(maxsize=None)
def _fixture(N, kind, variant):
    """A fixture of geary_cases.FIXTURES on the device: a SparseCounts ("counts") or a SparseExpression ("log")."""
    from gpzoo.likelihoods import SparseCounts
    if kind == "counts":
        return SparseCounts(torch.tensor(G.counts(N, variant))).cuda()
    return G.log_values(N, variant)[0].cuda()


def _sparse(N, kind):
    return _fixture(N, kind, M.FIXTURES[kind])


@functools.lru_cache(maxsize=None)
def _nbr(N, K):
    return torch.tensor(G.graph(N, K)).cuda()


@functools.lru_cache(maxsize=None)
def _perms(N):
    return torch.tensor(M.perms(N)).cuda()


def _i64(t):
    a = t.cpu().numpy()
    return a.view(np.int64).copy() if a.dtype == np.float64 else a.copy()


def _bits(r, fields=FIELDS):
    return [_i64(getattr(r, f)) for f in fields if getattr(r, f) is not None]


def _same_bits(a, b, msg=""):
    assert len(a) == len(b)
    for f, x, y in zip(FIELDS, a, b):
        np.testing.assert_array_equal(x, y, err_msg=f"{msg} {f}")


# ---- the sparse entry -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K", G.GRAPHS)
def test_the_sparse_entry_matches_the_oracles(N, K):
    """C within GEARY_ATOL_SPARSE, b2 and var within KURTOSIS_RTOL, the mean within fp64 epsilon x N x max |x| (the bound of
    a sum of N terms), the NaN pattern the oracle's, I the bits of gene_morans_i_sparse -- on every fixture, row kind and graph."""
    from gpzoo_amd import ops
    nbr = _nbr(N, K)
    for kind, variant in Y.FIXTURES:
        v, X = _fixture(N, kind, variant), Y.values(N, kind, variant)
        s = ops.gene_spatial_stats_sparse(v, nbr)
        assert all(getattr(s, f).shape == (G.D,) and getattr(s, f).dtype == torch.float64 and getattr(s, f).is_cuda
                   for f in ("I", "C", "mean", "var", "kurtosis"))
        np.testing.assert_array_equal(_i64(s.I), _i64(ops.gene_morans_i_sparse(v, nbr)))
        want, mom = Y.geary_oracle(X, G.graph(N, K)), Y.kurtosis_oracle(X)
        nan = np.isnan(want)
        assert nan[G.row_kinds(N)["empty"]] and not nan.all()
        C, b2 = s.C.cpu().numpy(), s.kurtosis.cpu().numpy()
        for got in (C, b2, s.I.cpu().numpy()):
            np.testing.assert_array_equal(np.isnan(got), nan)
        print(N, K, kind, variant, "max |C - oracle|", np.abs(C - want)[~nan].max(), "max rel b2",
              (np.abs(b2 - mom["kurtosis"]) / mom["kurtosis"])[~nan].max())
        np.testing.assert_allclose(C[~nan], want[~nan], rtol=0, atol=Y.GEARY_ATOL_SPARSE)
        np.testing.assert_allclose(b2[~nan], mom["kurtosis"][~nan], rtol=Y.KURTOSIS_RTOL, atol=0)
        np.testing.assert_allclose(s.var.cpu().numpy(), mom["var"], rtol=Y.KURTOSIS_RTOL, atol=0)
        np.testing.assert_allclose(s.mean.cpu().numpy(), mom["mean"], rtol=0, atol=np.finfo(np.float64).eps * N * np.abs(X).max())
        if K == N - 1:                                                  # the complete graph: C = 1 whatever the values
            np.testing.assert_allclose(C[~nan], 1.0, rtol=0, atol=Y.GEARY_ATOL_SPARSE)


def test_the_offset_of_a_sparse_expression_moves_the_mean_alone():
    from gpzoo.likelihoods import SparseExpression
    from gpzoo_amd import ops
    N, K = 1037, 6
    e = _fixture(N, "log", "full")
    offset = torch.linspace(-2.0, 3.0, G.D, dtype=torch.float64, device="cuda")
    a, b = ops.gene_spatial_stats_sparse(e, _nbr(N, K)), ops.gene_spatial_stats_sparse(SparseExpression(e.values, offset), _nbr(N, K))
    for f in ("I", "C", "var", "kurtosis"):
        np.testing.assert_array_equal(_i64(getattr(a, f)), _i64(getattr(b, f)), err_msg=f)
    plain = ops.gene_spatial_stats_sparse(e.values, _nbr(N, K))
    assert torch.equal(b.mean, plain.mean - offset) and torch.equal(a.mean, plain.mean - e.offset.cuda())


# ---- the dense-columns entry ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _columns(N, L):
    """(N, L) fp64: normal, count-like and nearly constant columns; column 0 of L > 1 is constant."""
    rng = np.random.default_rng(300 + 7 * N + L)
    V = rng.normal(size=(N, L)) * rng.uniform(0.1, 5.0, L) + rng.uniform(-3.0, 50.0, L)
    V[:, 1::3] = rng.poisson(0.3, size=V[:, 1::3].shape)
    if L > 1:
        V[:, 0] = 2.5
    V.setflags(write=False)
    return V


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("L", [1, 37, 65])
@pytest.mark.parametrize("N", [255, 256, 257, 513])
def test_the_dense_entry_matches_the_oracles(N, L, dtype):
    """C within GEARY_ATOL_ROWS, b2 and var within KURTOSIS_RTOL, I the bits of morans_i; across the 256-row chunk and beyond
    one 64-column tile."""
    from gpzoo_amd import ops
    V = torch.tensor(_columns(N, L)).to(dtype).cuda()
    X = V.cpu().double().numpy().T
    nbr = _nbr(N, DENSE_K)
    s = ops.spatial_stats(V, nbr)
    np.testing.assert_array_equal(_i64(s.I), _i64(ops.morans_i(V, nbr)))
    want, mom = Y.geary_oracle(X, G.graph(N, DENSE_K)), Y.kurtosis_oracle(X)
    nan = np.isnan(want)
    assert nan.sum() == (1 if L > 1 else 0)
    C, b2 = s.C.cpu().numpy(), s.kurtosis.cpu().numpy()
    np.testing.assert_array_equal(np.isnan(C), nan)
    np.testing.assert_array_equal(np.isnan(b2), nan)
    print(N, L, dtype, "max |C - oracle|", np.abs(C - want)[~nan].max())
    np.testing.assert_allclose(C[~nan], want[~nan], rtol=0, atol=Y.GEARY_ATOL_ROWS)
    np.testing.assert_allclose(b2[~nan], mom["kurtosis"][~nan], rtol=Y.KURTOSIS_RTOL, atol=0)
    np.testing.assert_allclose(s.var.cpu().numpy()[~nan], mom["var"][~nan], rtol=Y.KURTOSIS_RTOL, atol=0)
    np.testing.assert_allclose(s.mean.cpu().numpy(), mom["mean"], rtol=0, atol=np.finfo(np.float64).eps * N * np.abs(X).max())


@pytest.mark.parametrize("N,K", G.GRAPHS)
def test_the_dense_transpose_agrees_with_the_sparse_entry(N, K):
    from gpzoo_amd import ops
    for kind in sorted(M.FIXTURES):
        s = ops.gene_spatial_stats_sparse(_sparse(N, kind), _nbr(N, K))
        d = ops.spatial_stats(torch.tensor(M.dense(N, kind)).cuda().T.contiguous(), _nbr(N, K))
        a, b = s.C.cpu().numpy(), d.C.cpu().numpy()
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
        np.testing.assert_allclose(b, a, rtol=0, atol=Y.GEARY_ATOL_SPARSE + Y.GEARY_ATOL_ROWS, equal_nan=True)
        np.testing.assert_allclose(d.kurtosis.cpu().numpy(), s.kurtosis.cpu().numpy(), rtol=2 * Y.KURTOSIS_RTOL, atol=0, equal_nan=True)


# ---- permutations -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sorted(M.FIXTURES))
@pytest.mark.parametrize("N,K", G.GRAPHS)
def test_geary_sims_and_observed_match_the_oracles(N, K, kind):
    """sims within GEARY_ATOL_SPARSE of the oracle on the permuted dense array; the observed C the bits of the stats entry;
    NaN genes NaN throughout and counted nowhere."""
    from gpzoo_amd import ops
    v, nbr = _sparse(N, kind), _nbr(N, K)
    r = ops.gene_autocorr_perm_sparse(v, nbr, _perms(N), stat="geary", return_sims=True)
    assert r.stat == "geary" and r.sims.shape == (G.D, M.P) and r.sims.dtype == torch.float64
    np.testing.assert_array_equal(_i64(r.value), _i64(ops.gene_spatial_stats_sparse(v, nbr).C))
    want, sims = Y.sims_oracle(N, K, kind), r.sims.cpu().numpy()
    nan = np.isnan(Y.observed_oracle(N, K, kind))
    np.testing.assert_array_equal(np.isnan(sims), np.broadcast_to(nan[:, None], sims.shape))
    for t in (r.value, r.sim_mean, r.sim_m2):
        np.testing.assert_array_equal(np.isnan(t.cpu().numpy()), nan)
    assert not r.n_ge[torch.tensor(nan)].any() and not r.n_le[torch.tensor(nan)].any()
    print(N, K, kind, "max |sims - oracle|", np.abs(sims - want)[~nan].max())
    np.testing.assert_allclose(sims[~nan], want[~nan], rtol=0, atol=Y.GEARY_ATOL_SPARSE)
    np.testing.assert_allclose(r.sim_mean.cpu().numpy()[~nan], want[~nan].mean(axis=1), rtol=0, atol=Y.GEARY_ATOL_SPARSE)
    sd = want[~nan].std(axis=1)                                         # |var - var'| <= 2 sd e + e^2 for values within e
    np.testing.assert_array_less(np.abs((r.sim_m2 / M.P).cpu().numpy()[~nan] - want[~nan].var(axis=1)),
                                 2 * sd * Y.GEARY_ATOL_SPARSE + Y.GEARY_ATOL_SPARSE ** 2 + 1e-15)


@pytest.mark.parametrize("N,K", G.GRAPHS)
def test_geary_counts_are_exact_on_integer_data_and_inside_the_bracket_otherwise(N, K):
    from gpzoo_amd import ops
    r = ops.gene_autocorr_perm_sparse(_sparse(N, "counts"), _nbr(N, K), _perms(N), stat="geary")
    assert r.sims is None
    n_ge, n_le = Y.counts_oracle_exact(N, K)
    np.testing.assert_array_equal(r.n_ge.cpu().numpy(), n_ge)
    np.testing.assert_array_equal(r.n_le.cpu().numpy(), n_le)
    d = ops.autocorr_perm_rows(torch.tensor(M.dense(N, "counts")).cuda(), _nbr(N, K), _perms(N), stat="geary")
    np.testing.assert_array_equal(d.n_ge.cpu().numpy(), n_ge)
    np.testing.assert_array_equal(d.n_le.cpu().numpy(), n_le)
    if K == N - 1:                                                      # the complete graph: every permutation ties with C
        scored = ~np.isnan(Y.observed_oracle(N, K, "counts"))
        assert (r.n_ge.cpu().numpy()[scored] == M.P).all() and (r.n_le.cpu().numpy()[scored] == M.P).all()
    r = ops.gene_autocorr_perm_sparse(_sparse(N, "log"), _nbr(N, K), _perms(N), stat="geary")
    ge, le, band = Y.counts_bracket(N, K, "log")
    for got, lo in ((r.n_ge.cpu().numpy(), ge), (r.n_le.cpu().numpy(), le)):
        assert ((lo <= got) & (got <= lo + band)).all(), np.nonzero((lo > got) | (got > lo + band))[0]


@pytest.mark.parametrize("N,K,kind", [(1037, 6, "counts"), (1037, 6, "log"), (4099, 32, "log")])
def test_every_geary_output_is_independent_of_the_batch_and_of_the_lines_home(N, K, kind):
    from gpzoo_amd import ops
    v, nbr, perms = _sparse(N, kind), _nbr(N, K), _perms(N)
    first = _bits(ops.gene_autocorr_perm_sparse(v, nbr, perms, stat="geary", return_sims=True, perm_batch=1, line_mode="global"))
    for pb in (1, 3, 0):
        for mode in ("global", "lds"):
            _same_bits(first, _bits(ops.gene_autocorr_perm_sparse(v, nbr, perms, stat="geary", return_sims=True, perm_batch=pb,
                                                                  line_mode=mode)), f"perm_batch={pb} line_mode={mode}")
    dense = torch.tensor(M.dense(N, kind)).cuda()
    first = _bits(ops.autocorr_perm_rows(dense, nbr, perms, stat="geary", return_sims=True, perm_batch=1, line_mode="global"))
    for pb, mode in ((3, "lds"), (0, "global"), (0, "lds")):
        _same_bits(first, _bits(ops.autocorr_perm_rows(dense, nbr, perms, stat="geary", return_sims=True, perm_batch=pb, line_mode=mode)),
                   f"rows perm_batch={pb} line_mode={mode}")


@pytest.mark.parametrize("N,K", [(257, 1), (1037, 6), (1037, 32)])
def test_the_identity_permutation_reproduces_the_observed_c(N, K):
    from gpzoo_amd import ops
    perms = _perms(N).clone()
    perms[4] = torch.arange(N, dtype=torch.int32)
    for kind in sorted(M.FIXTURES):
        for mode in ("global", "lds"):
            r = ops.gene_autocorr_perm_sparse(_sparse(N, kind), _nbr(N, K), perms, stat="geary", return_sims=True, line_mode=mode)
            np.testing.assert_array_equal(_i64(r.sims[:, 4]), _i64(r.value))
        r = ops.autocorr_perm_rows(torch.tensor(M.dense(N, kind)).cuda(), _nbr(N, K), perms, stat="geary", return_sims=True)
        np.testing.assert_array_equal(_i64(r.sims[:, 4]), _i64(r.value))


@pytest.mark.parametrize("N,K", [(7, 6), (257, 6), (4099, 32)])
def test_stat_moran_returns_the_bits_of_the_moran_entries(N, K):
    from gpzoo_amd import ops
    for kind in sorted(M.FIXTURES):
        v, dense = _sparse(N, kind), torch.tensor(M.dense(N, kind)).cuda()
        for mode in ("global", "lds"):
            a = ops.gene_autocorr_perm_sparse(v, _nbr(N, K), _perms(N), stat="moran", return_sims=True, line_mode=mode)
            b = ops.gene_morans_perm_sparse(v, _nbr(N, K), _perms(N), return_sims=True, line_mode=mode)
            assert a.stat == "moran"
            _same_bits(_bits(a), _bits(b, MORAN_FIELDS), f"sparse {kind} {mode}")
        a = ops.autocorr_perm_rows(dense, _nbr(N, K), _perms(N), stat="moran", return_sims=True)
        _same_bits(_bits(a), _bits(ops.morans_perm_rows(dense, _nbr(N, K), _perms(N), return_sims=True), MORAN_FIELDS), f"rows {kind}")


# ---- all 5040 relabellings ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("table", sorted(Y.ENUM_TABLES))
def test_mean_and_variance_over_all_relabellings_are_the_randomisation_moments(table):
    """mean_sim and var_sim of both statistics over the complete (5040, 7) table, through ``gene_autocorr(perms=)`` for the
    stored entries and through the rows entry: the analytic E and Var_R to ENUM_RTOL = 1e-9, far from the normality variance."""
    from gpzoo.likelihoods import SparseCounts
    from gpzoo.utilities import gene_autocorr
    from gpzoo_amd import ops
    nbr, perms = torch.tensor(Y.ENUM_TABLES[table]).cuda(), torch.tensor(Y.enum_perms()).cuda()
    genes, stored = torch.tensor(Y.ENUM_GENES).cuda(), SparseCounts(torch.tensor(Y.ENUM_GENES)).cuda()
    want = Y.moments(Y.ENUM_TABLES[table], Y.kurtosis_oracle(Y.ENUM_GENES)["kurtosis"])
    P = perms.shape[0]
    for stat, E, V, Vn in (("moran", want["EI"], want["VI_rand"], want["VI_norm"]), ("geary", 1.0, want["VC_rand"], want["VC_norm"])):
        g = gene_autocorr(stored, graph=nbr, perms=perms, mode=stat, assumption="randomisation")
        rows = ops.autocorr_perm_rows(genes, nbr, perms, stat=stat)
        for name, mean, var in (("sparse", g.mean_sim, g.var_sim), ("rows", rows.sim_mean, rows.sim_m2 / P)):
            print(table, stat, name, (mean.cpu().numpy() - E) / E, var.cpu().numpy() / V - 1)
            np.testing.assert_allclose(mean.cpu().numpy(), E, rtol=Y.ENUM_RTOL, atol=0, err_msg=f"{stat} {name}")
            np.testing.assert_allclose(var.cpu().numpy(), V, rtol=Y.ENUM_RTOL, atol=0, err_msg=f"{stat} {name}")
            assert (np.abs(var.cpu().numpy() / Vn - 1) > 0.09).all()
        assert g.n_perms == P and g.variance.shape == (3,)
        np.testing.assert_allclose(g.variance.cpu().numpy(), V, rtol=Y.ENUM_RTOL, atol=0)       # b2 of the device, analytic
        np.testing.assert_allclose(float(g.expected), E, rtol=1e-15)


# ---- robustness ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K", [(257, 6), (1037, 32)])
def test_the_same_bits_on_poisoned_and_stale_partials(N, K):
    from gpzoo_amd import ops
    v, dense = _sparse(N, "log"), torch.tensor(M.dense(N, "log")).cuda()
    cols = dense.T.contiguous()

    def run():
        s, c = ops.gene_spatial_stats_sparse(v, _nbr(N, K)), ops.spatial_stats(cols, _nbr(N, K))
        return ([_i64(getattr(t, f)) for t in (s, c) for f in ("I", "C", "mean", "var", "kurtosis")]
                + _bits(ops.gene_autocorr_perm_sparse(v, _nbr(N, K), _perms(N), stat="geary", return_sims=True, perm_batch=8))
                + _bits(ops.autocorr_perm_rows(dense, _nbr(N, K), _perms(N), stat="geary", return_sims=True, perm_batch=8)))
    first = run()
    again = run()
    ws = ops._workspace(v.device, 1)
    assert ws.numel() >= ops.autocorr_perm_plan(N, G.D, K, M.P, nnz=v.values.nnz, stat="geary", perm_batch=8)["partials_bytes"]
    assert ws.numel() >= ops.spatial_stats_plan(N, K, D=G.D, nnz=v.values.nnz)["partials_bytes"]
    ws.fill_(0xFF)
    poisoned = run()
    other = 1037 if N != 1037 else 257
    ops.gene_autocorr_perm_sparse(_sparse(other, "counts"), _nbr(other, 1), _perms(other), stat="geary")      # leftovers of another shape
    ops.spatial_stats(torch.tensor(M.dense(other, "counts")).cuda().T.contiguous(), _nbr(other, 1))
    stale = run()
    for name, rerun in (("again", again), ("poisoned", poisoned), ("stale", stale)):
        for a, b in zip(first, rerun):
            np.testing.assert_array_equal(a, b, err_msg=name)


def test_a_bad_table_and_a_bad_permutation_raise_the_existing_errors():
    from gpzoo_amd import ops
    N, K = 257, 6
    v, dense = _sparse(N, "counts"), torch.tensor(M.dense(N, "counts")).cuda()
    clean = _bits(ops.gene_autocorr_perm_sparse(v, _nbr(N, K), _perms(N), stat="geary", return_sims=True))
    for name, entry in (("twice", 7), ("beyond", N), ("negative", -1)):
        perms = _perms(N).to(torch.int64)
        perms[11, 100] = perms[11, 7] if name == "twice" else entry
        for mode in ("global", "lds"):
            with pytest.raises(ValueError, match="not a permutation"):
                ops.gene_autocorr_perm_sparse(v, _nbr(N, K), perms, stat="geary", line_mode=mode)
        with pytest.raises(ValueError, match="not a permutation"):
            ops.autocorr_perm_rows(dense, _nbr(N, K), perms, stat="geary")
    nbr = _nbr(N, K).clone()
    nbr[200, 3] = 200
    for call in (lambda: ops.gene_autocorr_perm_sparse(v, nbr, _perms(N), stat="geary"),
                 lambda: ops.autocorr_perm_rows(dense, nbr, _perms(N), stat="geary"),
                 lambda: ops.gene_spatial_stats_sparse(v, nbr), lambda: ops.spatial_stats(dense.T.contiguous(), nbr)):
        with pytest.raises(ValueError, match="naming its own row"):
            call()
    nbr[200, 3] = N
    with pytest.raises(ValueError, match="naming its own row"):
        ops.gene_spatial_stats_sparse(v, nbr)
    _same_bits(clean, _bits(ops.gene_autocorr_perm_sparse(v, _nbr(N, K), _perms(N), stat="geary", return_sims=True)), "after the errors")


def test_one_gene_one_permutation_and_no_sims():
    from gpzoo.likelihoods import SparseCounts
    from gpzoo_amd import ops
    N, K = 257, 6
    Y_, nbr, perms = M.dense(N, "counts"), _nbr(N, K), _perms(N)
    full = ops.gene_autocorr_perm_sparse(_sparse(N, "counts"), nbr, perms, stat="geary", return_sims=True)
    d = G.D - 1
    one = ops.gene_autocorr_perm_sparse(SparseCounts(torch.tensor(Y_[d:d + 1])).cuda(), nbr, perms[:1], stat="geary")
    assert one.sims is None and one.value.shape == (1,)
    assert torch.equal(one.value, full.value[d:d + 1]) and torch.equal(one.sim_mean, full.sims[d:d + 1, 0])
    assert not one.sim_m2.any() and int(one.n_ge + one.n_le) >= 1
    s = ops.gene_spatial_stats_sparse(SparseCounts(torch.tensor(Y_[d:d + 1])).cuda(), nbr)
    assert torch.equal(s.C, full.value[d:d + 1])
