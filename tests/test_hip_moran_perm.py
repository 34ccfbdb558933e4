"""GPU: the permutation null of Moran's I (gpzoo_amd/csrc/moran_perm.hip) against the oracles of tests/moran_perm_cases.py --
the simulated I of every gene and permutation within the project's 1e-10 for this expression, the observed I with the bits
of gpz_gene_morans_i_sparse, the counts behind the p-values exactly (integer data) or inside the fp64 oracle's bracket, every
output with the same bits whatever the batch, the line's home and the scratch memory's contents, and the public path."""
import functools

import numpy as np
import pytest
import torch

import gene_rank_cases as G
import moran_perm_cases as M

pytestmark = pytest.mark.gpu

FIELDS = ("I", "n_ge", "n_le", "sim_mean", "sim_m2", "sims")


@functools.lru_cache(maxsize=None)
def _sparse(N, kind):
    """The fixture on the device: a SparseCounts ("counts") or the SparseExpression of its log-normalised values ("log")."""
    from gpzoo.likelihoods import SparseCounts
    if kind == "counts":
        return SparseCounts(torch.tensor(M.dense(N, kind))).cuda()
    return G.log_values(N, M.FIXTURES[kind])[0].cuda()


@functools.lru_cache(maxsize=None)
def _nbr(N, K):
    return torch.tensor(G.graph(N, K)).cuda()


@functools.lru_cache(maxsize=None)
def _perms(N):
    return torch.tensor(M.perms(N)).cuda()


def _bits(r):
    """Every output of a MoransPerm as integers (NaN payloads included)."""
    out = []
    for f in FIELDS:
        t = getattr(r, f)
        if t is not None:
            a = t.cpu().numpy()
            out.append(a.view(np.int64).copy() if a.dtype == np.float64 else a.copy())
    return out


def _same_bits(a, b, msg=""):
    assert len(a) == len(b)
    for f, x, y in zip(FIELDS, a, b):
        np.testing.assert_array_equal(x, y, err_msg=f"{msg} {f}")


@pytest.mark.parametrize("kind", sorted(M.FIXTURES))
@pytest.mark.parametrize("N,K", G.GRAPHS)
def test_sims_observed_and_moments_match_the_oracles(N, K, kind):
    """sims: rtol = 0, atol = 1e-10; I: the bits of gene_morans_i_sparse; NaN genes NaN throughout; the mean and the
    population variance of the simulations against numpy on the oracle's, 1e-10 absolute."""
    from gpzoo_amd import ops
    v, nbr = _sparse(N, kind), _nbr(N, K)
    r = ops.gene_morans_perm_sparse(v, nbr, _perms(N), return_sims=True)
    assert r.sims.shape == (G.D, M.P) and r.sims.dtype == torch.float64 and r.sims.is_cuda
    assert all(getattr(r, f).shape == (G.D,) for f in FIELDS[:5]) and r.n_ge.dtype == torch.int32 and r.n_le.dtype == torch.int32
    np.testing.assert_array_equal(r.I.cpu().numpy().view(np.int64), ops.gene_morans_i_sparse(v, nbr).cpu().numpy().view(np.int64))
    want, sims = M.sims_oracle(N, K, kind), r.sims.cpu().numpy()
    nan = np.isnan(M.observed_oracle(N, K, kind))
    assert nan[G.row_kinds(N)["empty"]] and not nan.all()
    np.testing.assert_array_equal(np.isnan(sims), np.broadcast_to(nan[:, None], sims.shape))
    for t in (r.I, r.sim_mean, r.sim_m2):
        np.testing.assert_array_equal(np.isnan(t.cpu().numpy()), nan)
    assert not r.n_ge[torch.tensor(nan)].any() and not r.n_le[torch.tensor(nan)].any()
    print(N, K, kind, "max |sims - oracle|", np.abs(sims - want)[~nan].max())
    np.testing.assert_allclose(sims[~nan], want[~nan], rtol=0, atol=G.MORAN_ATOL)
    np.testing.assert_allclose(r.sim_mean.cpu().numpy()[~nan], want[~nan].mean(axis=1), rtol=0, atol=1e-10)
    np.testing.assert_allclose((r.sim_m2 / M.P).cpu().numpy()[~nan], want[~nan].var(axis=1), rtol=0, atol=1e-10)


@pytest.mark.parametrize("N,K", G.GRAPHS)
def test_counts_are_exact_on_integer_data_and_inside_the_bracket_otherwise(N, K):
    from gpzoo_amd import ops
    r = ops.gene_morans_perm_sparse(_sparse(N, "counts"), _nbr(N, K), _perms(N))
    assert r.sims is None
    n_ge, n_le = M.counts_oracle_exact(N, K)
    np.testing.assert_array_equal(r.n_ge.cpu().numpy(), n_ge)
    np.testing.assert_array_equal(r.n_le.cpu().numpy(), n_le)
    if K == N - 1:                                                   # the complete graph: every permutation ties with I
        scored = ~np.isnan(M.observed_oracle(N, K, "counts"))
        assert (r.n_ge.cpu().numpy()[scored] == M.P).all() and (r.n_le.cpu().numpy()[scored] == M.P).all()
    r = ops.gene_morans_perm_sparse(_sparse(N, "log"), _nbr(N, K), _perms(N))
    ge, le, band = M.counts_bracket(N, K, "log")
    for got, lo in ((r.n_ge.cpu().numpy(), ge), (r.n_le.cpu().numpy(), le)):
        assert ((lo <= got) & (got <= lo + band)).all(), np.nonzero((lo > got) | (got > lo + band))[0]


@pytest.mark.parametrize("N,K,kind", [(1037, 6, "counts"), (1037, 6, "log"), (4099, 32, "log")])
def test_every_output_is_independent_of_the_batch_and_of_the_lines_home(N, K, kind):
    """perm_batch 1, 8 (19 = 8 + 8 + 3) and the plan's own (16 + 3 in LDS, 8 otherwise), the line in the scratch memory and in
    LDS: the same bits."""
    from gpzoo_amd import ops
    v, nbr, perms = _sparse(N, kind), _nbr(N, K), _perms(N)
    assert ops.morans_perm_plan(N, G.D, K, M.P, nnz=v.nnz if kind == "counts" else v.values.nnz)["perm_batch"] == 16
    first = _bits(ops.gene_morans_perm_sparse(v, nbr, perms, return_sims=True, perm_batch=1, line_mode="global"))
    for pb in (1, 8, 0, 19):
        for mode in ("global", "lds"):
            _same_bits(first, _bits(ops.gene_morans_perm_sparse(v, nbr, perms, return_sims=True, perm_batch=pb, line_mode=mode)),
                       f"perm_batch={pb} line_mode={mode}")
    dense = torch.tensor(M.dense(N, kind)).cuda()
    first = _bits(ops.morans_perm_rows(dense, nbr, perms, return_sims=True, perm_batch=1, line_mode="global"))
    for pb, mode in ((8, "lds"), (0, "global"), (0, "lds")):
        _same_bits(first, _bits(ops.morans_perm_rows(dense, nbr, perms, return_sims=True, perm_batch=pb, line_mode=mode)),
                   f"rows perm_batch={pb} line_mode={mode}")


@pytest.mark.parametrize("N,K", [(257, 1), (1037, 6), (1037, 32)])
def test_the_identity_permutation_reproduces_the_observed_bits(N, K):
    from gpzoo_amd import ops
    perms = _perms(N).clone()
    perms[4] = torch.arange(N, dtype=torch.int32)
    for kind in sorted(M.FIXTURES):
        for mode in ("global", "lds"):
            r = ops.gene_morans_perm_sparse(_sparse(N, kind), _nbr(N, K), perms, return_sims=True, line_mode=mode)
            np.testing.assert_array_equal(r.sims[:, 4].cpu().numpy().view(np.int64), r.I.cpu().numpy().view(np.int64))
        r = ops.morans_perm_rows(torch.tensor(M.dense(N, kind)).cuda(), _nbr(N, K), perms, return_sims=True)
        np.testing.assert_array_equal(r.sims[:, 4].cpu().numpy().view(np.int64), r.I.cpu().numpy().view(np.int64))


@pytest.mark.parametrize("N,K", G.GRAPHS)
def test_the_dense_rows_entry_agrees_with_the_sparse_one(N, K):
    """The same data as a dense (D, N) array: sims within 1e-10 of the sparse entry (the sums run over every spot, zeros
    included, in another order), the counts equal on the integer fixture."""
    from gpzoo_amd import ops
    for kind in sorted(M.FIXTURES):
        s = ops.gene_morans_perm_sparse(_sparse(N, kind), _nbr(N, K), _perms(N), return_sims=True)
        d = ops.morans_perm_rows(torch.tensor(M.dense(N, kind)).cuda(), _nbr(N, K), _perms(N), return_sims=True)
        a, b = s.sims.cpu().numpy(), d.sims.cpu().numpy()
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
        np.testing.assert_allclose(b, a, rtol=0, atol=G.MORAN_ATOL, equal_nan=True)
        np.testing.assert_allclose(d.I.cpu().numpy(), s.I.cpu().numpy(), rtol=0, atol=G.MORAN_ATOL, equal_nan=True)
        if kind == "counts":
            assert torch.equal(s.n_ge, d.n_ge) and torch.equal(s.n_le, d.n_le)


def test_a_bad_permutation_and_a_bad_table_raise_distinct_errors():
    """Argument errors reported through info; the kernels skip what is out of range.  The clean call still gives the clean
    answer afterwards."""
    from gpzoo_amd import ops
    N, K = 257, 6
    v, dense = _sparse(N, "counts"), torch.tensor(M.dense(N, "counts")).cuda()
    clean = _bits(ops.gene_morans_perm_sparse(v, _nbr(N, K), _perms(N), return_sims=True))
    for name, entry in (("twice", 7), ("beyond", N), ("negative", -1), ("wide", (1 << 32) + 5)):
        perms = _perms(N).to(torch.int64)
        perms[11, 100] = perms[11, 7] if name == "twice" else entry
        for mode in ("global", "lds"):
            with pytest.raises(ValueError, match="not a permutation"):
                ops.gene_morans_perm_sparse(v, _nbr(N, K), perms, line_mode=mode)
        with pytest.raises(ValueError, match="not a permutation"):
            ops.morans_perm_rows(dense, _nbr(N, K), perms)
    nbr = _nbr(N, K).clone()
    nbr[200, 3] = 200
    with pytest.raises(ValueError, match="naming its own row"):
        ops.gene_morans_perm_sparse(v, nbr, _perms(N))
    with pytest.raises(ValueError, match="naming its own row"):
        ops.morans_perm_rows(dense, nbr, _perms(N))
    from gpzoo.utilities import gene_autocorr
    with pytest.raises(ValueError, match="naming its own row"):
        gene_autocorr(v, graph=nbr, perms=_perms(N))
    _same_bits(clean, _bits(ops.gene_morans_perm_sparse(v, _nbr(N, K), _perms(N), return_sims=True)), "after the errors")


@pytest.mark.parametrize("N,K", [(257, 6), (1037, 32)])
def test_the_same_bits_on_poisoned_and_stale_scratch(N, K):
    from gpzoo_amd import ops
    v, dense = _sparse(N, "log"), torch.tensor(M.dense(N, "log")).cuda()

    def run():
        return (_bits(ops.gene_morans_perm_sparse(v, _nbr(N, K), _perms(N), return_sims=True, perm_batch=8))
                + _bits(ops.morans_perm_rows(dense, _nbr(N, K), _perms(N), return_sims=True, perm_batch=8)))
    first = run()
    again = run()
    ws = ops._workspace(v.device, 1)
    assert ws.numel() >= ops.morans_perm_plan(N, G.D, K, M.P, nnz=v.values.nnz, perm_batch=8)["partials_bytes"]
    ws.fill_(0xFF)
    poisoned = run()
    other = 1037 if N != 1037 else 257
    ops.gene_morans_perm_sparse(_sparse(other, "counts"), _nbr(other, 1), _perms(other))          # leftovers of another shape
    stale = run()
    for name, rerun in (("again", again), ("poisoned", poisoned), ("stale", stale)):
        for a, b in zip(first, rerun):
            np.testing.assert_array_equal(a, b, err_msg=name)


def test_one_gene_one_permutation_and_no_sims():
    from gpzoo.likelihoods import SparseCounts
    from gpzoo_amd import ops
    N, K = 257, 6
    Y, nbr, perms = M.dense(N, "counts"), _nbr(N, K), _perms(N)
    full = ops.gene_morans_perm_sparse(_sparse(N, "counts"), nbr, perms, return_sims=True)
    d = G.D - 1
    one = ops.gene_morans_perm_sparse(SparseCounts(torch.tensor(Y[d:d + 1])).cuda(), nbr, perms, return_sims=True)
    assert one.sims.shape == (1, M.P)
    for f in FIELDS:
        assert torch.equal(getattr(one, f), getattr(full, f)[d:d + 1]), f
    single = ops.gene_morans_perm_sparse(_sparse(N, "counts"), nbr, perms[:1], return_sims=True)
    assert single.sims.shape == (G.D, 1)
    ok = ~torch.isnan(full.I)
    assert torch.equal(single.sims[ok], full.sims[ok][:, :1]) and torch.equal(single.sim_mean[ok], full.sims[ok][:, 0])
    assert not single.sim_m2[ok].any() and bool(((single.n_ge + single.n_le)[ok] >= 1).all())
    quiet = ops.gene_morans_perm_sparse(_sparse(N, "counts"), nbr, perms)
    assert quiet.sims is None
    _same_bits(_bits(quiet), _bits(full)[:5])


def test_through_gene_autocorr():
    from gpzoo.utilities import GeneAutocorr, GeneAutocorrPerm, fdr_bh, gene_autocorr
    from gpzoo_amd import ops
    N, K = 1037, 6
    c, nbr, perms = _sparse(N, "counts"), _nbr(N, K), _perms(N)
    plain = gene_autocorr(c, graph=nbr)
    assert type(plain) is GeneAutocorr and len(plain) == 4
    np.testing.assert_array_equal(plain.I.cpu().numpy().view(np.int64), ops.gene_morans_i_sparse(c, nbr).cpu().numpy().view(np.int64))
    a, b = (gene_autocorr(c, graph=nbr, n_perms=19, seed=3, return_sims=True) for _ in range(2))
    assert type(a) is GeneAutocorrPerm and a.n_perms == 19 and a.sims.shape == (G.D, 19)
    for f in GeneAutocorrPerm._fields:
        x, y = getattr(a, f), getattr(b, f)
        assert x == y if f == "n_perms" else torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0)), f
    other = gene_autocorr(c, graph=nbr, n_perms=19, seed=4, return_sims=True)
    assert not torch.equal(torch.nan_to_num(other.sims), torch.nan_to_num(a.sims))
    for f in GeneAutocorr._fields:                                  # the first four fields: the call without permutations
        np.testing.assert_array_equal(getattr(a, f).cpu().numpy().view(np.int64), getattr(plain, f).cpu().numpy().view(np.int64))
    g = gene_autocorr(c, graph=nbr, perms=perms, return_sims=True)
    r = ops.gene_morans_perm_sparse(c, nbr, perms, return_sims=True)
    assert g.n_perms == M.P and torch.equal(g.n_ge, r.n_ge) and torch.equal(g.n_le, r.n_le)
    assert torch.equal(torch.nan_to_num(g.sims, nan=-7.0), torch.nan_to_num(r.sims, nan=-7.0))
    n_ge, n_le = M.counts_oracle_exact(N, K)
    nan = np.isnan(M.observed_oracle(N, K, "counts"))
    ulps = dict(rtol=4 * np.finfo(np.float64).eps, atol=0)          # one division on the device
    np.testing.assert_allclose(g.pval_greater.cpu().numpy()[~nan], (n_ge[~nan] + 1) / (M.P + 1), **ulps)
    np.testing.assert_allclose(g.pval_less.cpu().numpy()[~nan], (n_le[~nan] + 1) / (M.P + 1), **ulps)
    np.testing.assert_allclose(g.pval_sim.cpu().numpy()[~nan], (np.minimum(n_ge, n_le)[~nan] + 1) / (M.P + 1), **ulps)
    assert torch.equal(g.pval_sim[~torch.isnan(g.I)], torch.minimum(g.pval_greater, g.pval_less)[~torch.isnan(g.I)])
    sims = M.sims_oracle(N, K, "counts")[~nan]
    np.testing.assert_allclose(g.var_sim.cpu().numpy()[~nan], sims.var(axis=1), rtol=0, atol=1e-10)
    # z_sim = (I - mean) / sd: I and the mean within 1e-10 each, the variance within 1e-10 (sd within 1e-10 / (2 sd)), and
    # the last bits of the quotient; pval_z_sim has a slope of at most 0.4 (the normal density) in z
    sd = sims.std(axis=1)
    z = (M.observed_oracle(N, K, "counts")[~nan] - sims.mean(axis=1)) / sd
    z_bound = (2e-10 + np.abs(z) * 1e-10 / (2 * sd)) / sd + 1e-14 * np.abs(z)
    assert (np.abs(g.z_sim.cpu().numpy()[~nan] - z) <= z_bound).all()
    from math import erfc, sqrt
    want_p = np.array([0.5 * erfc(abs(t) / sqrt(2)) for t in z])
    assert (np.abs(g.pval_z_sim.cpu().numpy()[~nan] - want_p) <= 0.4 * z_bound + 1e-14 * want_p + 1e-300).all()
    for f in ("pval_greater", "pval_less", "pval_sim", "mean_sim", "var_sim", "z_sim", "pval_z_sim"):
        assert np.isnan(getattr(g, f).cpu().numpy()[nan]).all(), f
    assert not g.n_ge.cpu().numpy()[nan].any() and not g.n_le.cpu().numpy()[nan].any()
    q = fdr_bh(g.pval_sim)
    assert q.is_cuda and bool((q[~torch.isnan(q)] >= g.pval_sim[~torch.isnan(q)]).all()) and np.isnan(q.cpu().numpy()[nan]).all()
    # a dense tensor: I, expected, variance, z are those of the call without permutations; the counts those of the stored entries
    dense = torch.tensor(M.dense(N, "counts")).cuda()
    dp, d0 = gene_autocorr(dense, graph=nbr, perms=perms), gene_autocorr(dense, graph=nbr)
    for f in GeneAutocorr._fields:
        np.testing.assert_array_equal(getattr(dp, f).cpu().numpy().view(np.int64), getattr(d0, f).cpu().numpy().view(np.int64))
    assert dp.sims is None and torch.equal(dp.n_ge, g.n_ge) and torch.equal(dp.n_le, g.n_le)
