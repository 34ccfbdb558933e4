"""CPU: the oracles of tests/moran_perm_cases.py agree with each other, the band of the non-integer fixtures stays thin, and
relabelling the graph is permuting the values."""
import numpy as np
import pytest

import gene_rank_cases as G
import moran_perm_cases as M


@pytest.mark.parametrize("N,K", G.GRAPHS)
def test_the_exact_counts_lie_in_the_bracket_of_the_fp64_oracle(N, K):
    n_ge, n_le = M.counts_oracle_exact(N, K)
    ge, le, band = M.counts_bracket(N, K, "counts")
    assert ((ge <= n_ge) & (n_ge <= ge + band)).all(), np.nonzero((ge > n_ge) | (n_ge > ge + band))[0]
    assert ((le <= n_le) & (n_le <= le + band)).all(), np.nonzero((le > n_le) | (n_le > le + band))[0]
    kinds = G.row_kinds(N)
    assert n_ge[kinds["empty"]] == 0 and n_le[kinds["empty"]] == 0
    scored = ~np.isnan(M.observed_oracle(N, K, "counts"))
    assert ((n_ge + n_le >= M.P) == scored).all()                 # every permutation is >=, <= or both
    if K == N - 1:                                                # the complete graph: every permutation ties
        assert (n_ge[scored] == M.P).all() and (n_le[scored] == M.P).all()


def test_the_band_of_the_log_fixtures_is_thin():
    """At most 5 % of the (gene, permutation) pairs of a log-value fixture with N >= 257 lie within BAND of I: the bracket
    test on the device then pins nearly every comparison."""
    for N, K in G.GRAPHS:
        if N < 257:
            continue
        inside, pairs = M.band_share(N, K, "log")
        print(N, K, "in band", inside, "of", pairs)
        assert pairs > 0 and inside <= M.BAND_SHARE_MAX * pairs, (N, K, inside, pairs)


@pytest.mark.parametrize("kind", sorted(M.FIXTURES))
@pytest.mark.parametrize("N,K", G.GRAPHS)
def test_relabelling_the_graph_is_permuting_the_values(N, K, kind):
    X, nbr = M.dense(N, kind), G.graph(N, K)
    for pi in M.perms(N)[:3]:
        assert sorted(pi.tolist()) == list(range(N))
        want = G.moran_oracle(X[:, pi], nbr)
        got = G.moran_oracle(X, M.relabelled(nbr, pi))
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12, equal_nan=True)
    np.testing.assert_array_equal(M.relabelled(nbr, np.arange(N)), nbr)
