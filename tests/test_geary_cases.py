"""CPU: the infrastructure of tests/geary_cases.py checks itself -- the emulation of the sparse kernel's expression against
the direct oracle (which is where GEARY_ATOL_SPARSE comes from), the expansion identity in integers, the analytic
randomisation moments against the full enumeration of 7! relabellings, the band condition of the permutation counts on the
oracle alone, and ``utilities._autocorr_moments`` against the dense-W moments."""
import numpy as np
import pytest

import gene_rank_cases as G
import geary_cases as Y
import moran_perm_cases as M


def test_the_recorded_tolerances_are_what_the_docstring_says():
    assert Y.GEARY_ATOL_ROWS == G.MORAN_ATOL == 1e-10
    assert Y.GEARY_ATOL_SPARSE == 4.0 * Y.EMULATION_WORST <= 1e-9
    assert Y.KURTOSIS_RTOL == 1e-11 == G.DEVIANCE_RTOL and Y.BAND == 2.0 * Y.GEARY_ATOL_SPARSE


@pytest.mark.parametrize("N,K", G.GRAPHS)
def test_the_emulation_stays_within_a_quarter_of_the_sparse_bound(N, K):
    """|geary_expanded - geary_oracle| <= GEARY_ATOL_SPARSE / 4 on every fixture, and <= 1.1e-13 on the integer ones."""
    for kind, variant in Y.FIXTURES:
        err = Y.emulation_error(N, K, kind, variant)
        print(N, K, kind, variant, err)
        assert err <= Y.GEARY_ATOL_SPARSE / 4
        assert kind != "counts" or err <= 1.1e-13


def test_the_worst_emulation_error_is_the_every_spot_log_gene_at_the_largest_n():
    N = G.NS[-1]
    X = Y.values(N, "log", "full")
    worst = [int(np.nanargmax(np.abs(Y.geary_expanded(X, G.graph(N, K)) - Y.geary_oracle(X, G.graph(N, K))))) for K in G.KS]
    stats = Y.kurtosis_oracle(X)
    ratio = stats["mean"] ** 2 / np.where(stats["var"] > 0, stats["var"], np.inf)
    assert all(ratio[d] >= 0.5 * ratio.max() for d in worst), (worst, ratio[worst], ratio.max())


@pytest.mark.parametrize("N,K", G.GRAPHS)
def test_the_expansion_identity_is_exact_on_integer_data(N, K):
    """G = sum_i sum_j (x_i - x_j)^2 = K Q + Q_in - 2 C_s in integers, on both integer fixtures."""
    nbr = G.graph(N, K)
    indeg = np.bincount(nbr.reshape(-1), minlength=N).astype(np.int64)
    for variant in G.VARIANTS:
        X = G.counts(N, variant).astype(np.int64)
        direct = ((X[:, :, None] - X[:, nbr]) ** 2).sum(axis=(1, 2))
        Q, Qin, Cs = (X * X).sum(axis=1), (X * X * indeg).sum(axis=1), (X * X[:, nbr].sum(axis=2)).sum(axis=1)
        np.testing.assert_array_equal(direct, K * Q + Qin - 2 * Cs)
        for d in range(G.D):                                   # the fp64 sums of the emulation are exact here too
            nz = np.nonzero(X[d])[0]
            if nz.size:
                S, Qf, Cf, Qinf = Y.expansion_sums(X[d, nz].astype(np.float64), nz, X[d].astype(np.float64), nbr, indeg.astype(np.float64))
                assert (S, Qf, Cf, Qinf) == (X[d].sum(), Q[d], Cs[d], Qin[d])


@pytest.mark.parametrize("table", sorted(Y.ENUM_TABLES))
def test_the_randomisation_moments_are_the_moments_over_all_relabellings(table):
    """Mean and population variance of I and C over all 5040 relabellings equal E[I], Var_R[I], 1 and Var_R[C] to 1e-12
    relative; the normality variances differ from them by more than 10 %, so a test can tell the two apart -- in 17 of the
    18 (table, gene, statistic) combinations; for I of the log1p gene over the irregular table the gap is 9.94 %, which is
    still 1e8 times the 1e-9 the device test allows."""
    nbr = Y.ENUM_TABLES[table]
    assert Y.enum_perms().shape == (5040, 7) and (Y.enum_perms()[0] == np.arange(7)).all()
    assert len({tuple(p) for p in Y.enum_perms()}) == 5040
    b2 = Y.kurtosis_oracle(Y.ENUM_GENES)["kurtosis"]
    m = Y.moments(nbr, b2)
    for d, x in enumerate(Y.ENUM_GENES):
        I, C = Y.enum_statistics(x, nbr)
        np.testing.assert_allclose(I.mean(), m["EI"], rtol=1e-12)
        np.testing.assert_allclose(C.mean(), 1.0, rtol=1e-12)
        np.testing.assert_allclose(I.var(), m["VI_rand"][d], rtol=1e-12)
        np.testing.assert_allclose(C.var(), m["VC_rand"][d], rtol=1e-12)
        gaps = {"I": abs(m["VI_norm"] / m["VI_rand"][d] - 1), "C": abs(m["VC_norm"] / m["VC_rand"][d] - 1)}
        for stat, gap in gaps.items():
            assert gap > (0.099 if (table, d, stat) == ("irregular", 1, "I") else 0.1), (table, d, stat, gap)
    np.testing.assert_allclose(Y.geary_oracle(Y.ENUM_GENES, nbr), [Y.enum_statistics(x, nbr)[1][0] for x in Y.ENUM_GENES], rtol=1e-14)


@pytest.mark.parametrize("N,K", [g for g in G.GRAPHS if g[0] >= 257])
def test_the_oracle_alone_satisfies_the_band_condition(N, K):
    """At most BAND_SHARE_MAX of the (gene, permutation) pairs of the "log" fixture lie within BAND of the observed C."""
    inside, pairs = Y.band_share(N, K, "log")
    print(N, K, inside, pairs)
    assert pairs > 0 and inside <= M.BAND_SHARE_MAX * pairs


def test_the_integer_oracle_agrees_with_the_fp64_oracle_outside_the_band():
    N, K = 257, 6
    n_ge, n_le = Y.counts_oracle_exact(N, K)
    ge, le, band = Y.counts_bracket(N, K, "counts")
    assert ((ge <= n_ge) & (n_ge <= ge + band)).all() and ((le <= n_le) & (n_le <= le + band)).all()
    scored = ~np.isnan(Y.observed_oracle(N, K, "counts"))
    assert ((n_ge + n_le)[scored] >= M.P).all() and not n_ge[~scored].any() and not n_le[~scored].any()


@pytest.mark.parametrize("N,K", [(7, 1), (7, 6), (257, 6), (1037, 32)] + [(7, t) for t in sorted(Y.ENUM_TABLES)])
def test_autocorr_moments_match_the_dense_w_moments(N, K):
    """``utilities._autocorr_moments`` (integer counts of the table, exact rationals) against moments() (dense W, floats): 1e-12
    relative, 1e-15 absolute over the complete graph; its normality variance of I is ``_moran_moments``' within the same."""
    import torch
    from gpzoo_amd.utilities import _autocorr_moments, _moran_moments
    nbr = Y.ENUM_TABLES[K] if isinstance(K, str) else G.graph(N, K)
    K = nbr.shape[1]
    b2 = np.array([1.0, 1.7, 3.0, 40.0, 4000.0])
    got, want = _autocorr_moments(torch.tensor(nbr), torch.tensor(b2)), Y.moments(nbr, b2)
    assert float(got["EI"]) == want["EI"] and float(got["EC"]) == 1.0
    for key in ("VI_norm", "VC_norm", "VI_rand", "VC_rand"):
        g, w = got[key].numpy(), np.asarray(want[key])
        assert g.shape == w.shape and g.dtype == np.float64
        assert (np.abs(g - w) <= Y.moments_bound(N, K, w)).all(), (key, g, w)
    assert abs(float(_moran_moments(torch.tensor(nbr))[1]) - float(got["VI_norm"])) <= G.moments_bound(N, K, want["VI_norm"])
    assert "VI_rand" not in _autocorr_moments(torch.tensor(nbr))
    if N < 4:
        return
    with pytest.raises(ValueError, match="N >= 4"):
        _autocorr_moments(torch.tensor([[1], [2], [0]]), torch.tensor(b2))
