"""CPU: the cases of tests/gene_rank_cases.py hit every boundary tests/test_hip_gene_rank.py is meant to run, their oracles
are finite or NaN exactly where stated, and the expanded form of Moran's I that the kernel evaluates, written in numpy with
sequential fp64 sums, stays inside the GPU test's bound on every case -- so that bound is one the formula can meet."""
import numpy as np
import pytest

import gene_rank_cases as G


@pytest.fixture(scope="module", autouse=True)
def _library():
    from gpzoo_amd import build
    build.build(force=False, verbose=False)


def test_shapes_are_the_ones_named_and_off_the_tile():
    assert G.NS == (7, 257, 1037, 4099) and G.KS == (1, 6, 32) and G.D == 37
    assert all(N % 64 for N in G.NS)
    assert sorted(K for N, K in G.GRAPHS if N == 7) == [1, 6]
    assert all(sorted(K for N, K in G.GRAPHS if N == n) == [1, 6, 32] for n in G.NS[1:])
    g = G.granularity()
    assert g >= 64 and g % 64 == 0
    assert G.NS[-1] > 4 * g                           # a row stored at every spot spans several sweeps


@pytest.mark.parametrize("N", G.NS)
def test_counts_hit_every_row_kind(N):
    g = G.granularity()
    kinds = G.row_kinds(N)
    full, cut = G.counts(N, "full"), G.counts(N, "holes")
    assert full.shape == (G.D, N) and full.dtype == np.float32 and (full >= 0).all() and (full == np.round(full)).all()
    nnz = (full != 0).sum(axis=1)
    assert nnz[kinds["empty"]] == 0 and nnz[kinds["one"]] == 1
    assert nnz[kinds["every"]] == N and len(set(full[kinds["every"]])) > 1
    assert nnz[kinds["constant"]] == N and len(set(full[kinds["constant"]])) == 1
    if N >= g + 1:
        assert [nnz[kinds[k]] for k in ("g-1", "g+0", "g+1")] == [g - 1, g, g + 1]
    else:
        assert not any(k.startswith("g") for k in kinds)
    assert set(np.nonzero(full[kinds["mutual"]])[0]) == {0, 1}
    assert set(np.nonzero(full[kinds["unnamed"]])[0]) == set(range(N - G.UNNAMED, N))
    assert (full.sum(axis=0) > 0).all()               # "full": every spot has counts ...
    empty = np.nonzero(cut.sum(axis=0) == 0)[0]
    assert set(empty) == set(G.holes(N)) and len(empty) >= 1      # ... "holes": spots with no counts at all
    assert (cut[:, np.setdiff1d(np.arange(N), empty)] == full[:, np.setdiff1d(np.arange(N), empty)]).all()
    rates = full[9:].mean(axis=1)
    assert rates.max() > 200 and full.max() < 2 ** 24 and (full[9:12] == 0).mean() > 0.9     # rates 0.002 ... 400


def test_the_g_rows_exist_from_the_second_shape_on():
    g = G.granularity()
    assert [N >= g + 1 for N in G.NS] == [False, True, True, True]


@pytest.mark.parametrize("N,K", G.GRAPHS)
def test_graph_is_a_valid_table_with_mutual_and_unnamed_spots(N, K):
    nbr = G.graph(N, K)
    assert nbr.shape == (N, K) and nbr.dtype == np.int64 and nbr.min() >= 0 and nbr.max() < N
    assert not (nbr == np.arange(N)[:, None]).any()
    s = np.sort(nbr, axis=1)
    assert not (s[:, 1:] == s[:, :-1]).any()
    assert 1 in nbr[0] and 0 in nbr[1]
    indeg = np.bincount(nbr.reshape(-1), minlength=N)
    u = G.n_unnamed(N, K)
    assert (u == 0) == ((N, K) == (7, 6))             # the complete graph names everybody
    assert (indeg[N - u:] == 0).all() if u else (indeg > 0).all()


@pytest.mark.parametrize("N,K", G.GRAPHS)
def test_moran_oracle_is_nan_where_stated_and_the_expanded_form_meets_the_bound(N, K):
    nbr = G.graph(N, K)
    kinds = G.row_kinds(N)
    for variant in G.VARIANTS:
        for raw, dense in ((True, G.counts(N, variant)), (False, G.log_values(N, variant)[1])):
            want = G.moran_oracle(dense, nbr)
            nnz = (dense != 0).sum(axis=1)
            nan = (nnz == 0) | ((nnz == N) & (dense.min(axis=1) == dense.max(axis=1)))
            # one count at every spot is constant; its log-normalised values follow the spots' sizes and are not
            assert nan[kinds["empty"]] and nan[kinds["constant"]] == (raw and variant == "full")
            np.testing.assert_array_equal(np.isnan(want), nan)
            assert np.isfinite(want[~nan]).all() and (np.abs(want[~nan]) <= 1.5).all()
            got = G.moran_expanded(dense, nbr)
            np.testing.assert_array_equal(np.isnan(got), nan)
            err = np.abs(got - want)[~nan].max()
            print(N, K, variant, dense.dtype, "expanded form vs oracle", err)
            assert err <= G.MORAN_ATOL


@pytest.mark.parametrize("N", G.NS)
def test_deviance_oracle_is_finite_and_zero_for_an_empty_gene(N):
    kinds = G.row_kinds(N)
    for variant in G.VARIANTS:
        Y = G.counts(N, variant)
        for family, which in (("poisson", "totals"), ("poisson", "factors"), ("binomial", "totals")):
            o = G.deviance_oracle(Y, G.sizes(N, variant, which), family)
            assert all(np.isfinite(v).all() for v in o.values())
            assert o["deviance"][kinds["empty"]] == 0 and o["count"][kinds["empty"]] == 0
            np.testing.assert_array_equal(o["sum"], Y.astype(np.float64).sum(axis=1))
            assert (o["scale"] >= np.abs(o["deviance"]) * (1 - 1e-12)).all()
            if which == "totals":
                assert (o["deviance"] >= -1e-9 * o["scale"]).all()        # a deviance against its own totals


@pytest.mark.parametrize("N,K", [g for g in G.GRAPHS if g[0] <= 1037])
def test_moments_oracle_matches_the_closed_form_counts(N, K):
    nbr = G.graph(N, K)
    EI, VI = G.moments_oracle(nbr)
    assert EI == -1.0 / (N - 1) and np.isfinite(VI)
    edges = {(i, int(j)) for i in range(N) for j in nbr[i]}
    m = sum((j, i) in edges for i, j in edges) // 2
    indeg = np.bincount(nbr.reshape(-1), minlength=N)
    S1, S2 = (N * K + 2 * m) / K ** 2, ((1 + indeg / K) ** 2).sum()
    closed = (N * N * S1 - N * S2 + 3.0 * N * N) / ((N * N - 1.0) * N * N) - EI * EI
    assert m >= 1 and abs(closed - VI) <= G.moments_bound(N, K, VI)
    assert (VI > 1e-6) == ((N, K) != (7, 6))
