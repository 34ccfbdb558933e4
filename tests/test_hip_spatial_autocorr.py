"""GPU: the self-kNN graph (gpz_spatial_knn) equals the brute-force oracle exactly, Moran's I (gpz_morans_i) matches
the fp64 oracle and is bitwise reproducible, and dims_autocorr behaves as the reference's squidpy path."""
import numpy as np
import pytest
import torch

import spatial_oracle as O

pytestmark = pytest.mark.gpu


def _graph(X, K):
    from gpzoo_amd import ops
    idx = ops.spatial_knn(torch.as_tensor(X).cuda(), K)
    assert idx.dtype == torch.int64 and idx.shape == (X.shape[0], K)
    return idx.cpu().numpy()


def _points(N, d, seed):
    rng = np.random.default_rng(seed)
    return rng.random((N, d)) * 10.0 - 5.0


@pytest.mark.parametrize("N,d,K,dtype", [
    (7, 2, 6, np.float32), (2, 1, 1, np.float64), (33, 4, 32, np.float64),
    (257, 1, 6, np.float64), (257, 2, 32, np.float32), (257, 3, 1, np.float64),
    (4099, 2, 6, np.float64), (4099, 3, 32, np.float32), (4099, 4, 6, np.float32), (4099, 1, 32, np.float32),
    (70001, 2, 6, np.float32), (70001, 3, 6, np.float64), (70001, 4, 1, np.float64), (70001, 1, 6, np.float64),
])
def test_graph_equals_oracle(N, d, K, dtype):
    X = _points(N, d, N + 7 * d + K).astype(dtype)
    got = _graph(X, K)
    rows = np.arange(N) if N <= 4099 else np.random.default_rng(1).choice(N, 1024, replace=False)
    np.testing.assert_array_equal(got[rows], O.knn_rows(X, K, rows))


@pytest.mark.parametrize("K", [1, 6, 32])
def test_graph_on_a_lattice_breaks_exact_ties_by_index(K):
    g = np.arange(64, dtype=np.float64)
    X = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    X = X[np.random.default_rng(3).permutation(len(X))]          # index order unrelated to position
    np.testing.assert_array_equal(_graph(X.astype(np.float32), K), O.knn_rows(X, K))


def test_graph_with_triplicated_points():
    base = _points(700, 2, 5)
    X = np.concatenate([base, base, base])[np.random.default_rng(4).permutation(2100)]
    got = _graph(X, 6)
    np.testing.assert_array_equal(got, O.knn_rows(X, 6))
    d2 = ((X[got[:, :2]] - X[:, None]) ** 2).sum(-1)
    assert (d2 == 0).all()                                       # the two copies come first


@pytest.mark.parametrize("K", [1, 6, 32])
def test_graph_of_identical_points_takes_the_lowest_other_indices(K):
    N = 300
    got = _graph(np.full((N, 3), 1.25), K)
    want = np.array([[j for j in range(K + 1) if j != i][:K] for i in range(N)])
    np.testing.assert_array_equal(got, want)


def test_graph_at_scale():
    """N = 200 000: a uniform disc plus dense clusters; 2 048 sampled rows against the oracle, every row checked."""
    rng = np.random.default_rng(11)
    n_disc = 150_000
    r, t = np.sqrt(rng.random(n_disc)) * 100.0, rng.random(n_disc) * 2 * np.pi
    disc = np.stack([r * np.cos(t), r * np.sin(t)], 1)
    centres = rng.random((25, 2)) * 160.0 - 80.0
    clusters = centres[rng.integers(0, 25, 50_000)] + rng.normal(size=(50_000, 2)) * 0.05
    X = np.concatenate([disc, clusters])[rng.permutation(200_000)].astype(np.float32)
    N, K = len(X), 6
    got = _graph(X, K)
    rows = rng.choice(N, 2048, replace=False)
    np.testing.assert_array_equal(got[rows], O.knn_rows(X, K, rows))
    assert got.min() >= 0 and got.max() < N
    assert not (got == np.arange(N)[:, None]).any()
    s = np.sort(got, axis=1)
    assert not (s[:, 1:] == s[:, :-1]).any()


def test_graph_independent_of_the_search_order():
    """The C entry with the identity, a random permutation and a table that is no permutation (replaced on the
    device by the identity): the same graph."""
    from gpzoo_amd import _lib, ops
    lib = _lib.load()
    X = torch.as_tensor(_points(3000, 2, 8)).cuda()
    N, K = 3000, 6
    want = ops.spatial_knn(X, K)
    ws = torch.empty(lib.gpz_spatial_knn_workspace_bytes(N, 2, K), dtype=torch.uint8, device="cuda")
    bad = torch.arange(N, device="cuda")
    bad[5] = 7
    for order in (None, torch.randperm(N, device="cuda"), bad, bad - N):
        idx = torch.empty((N, K), dtype=torch.int64, device="cuda")
        rc = lib.gpz_spatial_knn(ops._ptr(X), N, 2, K, _lib.GPZ_F64, ops._ptr(order), ops._ptr(idx), ops._ptr(ws),
                                 ws.numel(), ops._stream(X.device))
        _lib.check(rc, "gpz_spatial_knn")
        assert torch.equal(idx, want)


@pytest.mark.parametrize("L", [1, 20, 33])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_morans_i_matches_oracle_and_is_reproducible(L, dtype):
    from gpzoo_amd import ops
    rng = np.random.default_rng(L)
    X = _points(5000, 2, 2)
    V = np.sin(X[:, :1] * rng.random(L)) + 0.3 * rng.normal(size=(5000, L)) + 3.0
    V = torch.as_tensor(V).to(dtype)
    nbr = ops.spatial_knn(torch.as_tensor(X).cuda(), 6)
    I1 = ops.morans_i(V.cuda(), nbr)
    I2 = ops.morans_i(V.cuda(), nbr)
    assert I1.dtype == torch.float64 and I1.shape == (L,)
    assert torch.equal(I1, I2)
    want = O.morans_i(V.double().numpy(), nbr.cpu().numpy())
    np.testing.assert_allclose(I1.cpu().numpy(), want, rtol=0, atol=1e-10)


def test_morans_i_rejects_a_corrupted_table():
    from gpzoo_amd import ops
    X = torch.as_tensor(_points(500, 2, 9)).cuda()
    V = torch.randn(500, 3, dtype=torch.float64, device="cuda")
    nbr = ops.spatial_knn(X, 6)
    for i, j, v in [(10, 2, 500), (11, 0, -1), (12, 5, 12)]:
        bad = nbr.clone()
        bad[i, j] = v
        with pytest.raises(ValueError, match="neighbour table"):
            ops.morans_i(V, bad)
    ops.morans_i(V, nbr)                         # the clean table still passes


def _field(N, seed):
    rng = np.random.default_rng(seed)
    X = rng.random((N, 2))
    smooth = np.sin(2 * np.pi * X[:, 0]) + np.cos(2 * np.pi * X[:, 1])
    return X, smooth, rng.normal(size=N)


def test_dims_autocorr_smooth_noise_constant():
    from gpzoo.utilities import dims_autocorr
    X, smooth, noise = _field(20_000, 1)
    F = np.stack([noise, np.full(len(X), 0.1), smooth], axis=1)
    idx, I = dims_autocorr(F, X)
    assert idx.dtype == np.int64 and I.dtype == np.float64
    assert idx.tolist() == [2, 0, 1]
    assert I[0] > 0.99 and abs(I[1]) < 0.02 and np.isnan(I[2])
    want = O.morans_i(F, _graph(X, 6))
    np.testing.assert_allclose(I[:2], want[[2, 0]], rtol=0, atol=1e-10)


def test_dims_autocorr_orders():
    from gpzoo.utilities import dims_autocorr
    X, smooth, noise = _field(3000, 2)
    F = np.stack([noise, smooth, noise, smooth, noise], axis=1)     # equal values stay in column order
    idx, I = dims_autocorr(F, X)
    assert idx.tolist() == [1, 3, 0, 2, 4]
    assert I[0] == I[1] and I[2] == I[3] == I[4]
    rng = np.random.default_rng(5)
    F12 = smooth[:, None] * rng.random(12) + rng.normal(size=(3000, 12)) * rng.random(12)
    idx_u, I_u = dims_autocorr(F12, X, sort=False)
    assert idx_u.tolist() == [0, 1, 10, 11, 2, 3, 4, 5, 6, 7, 8, 9]
    idx_s, I_s = dims_autocorr(F12, X)
    np.testing.assert_array_equal(I_u, I_s[np.argsort(idx_s)][idx_u])
    assert (np.diff(I_s) <= 0).all()


def test_dims_autocorr_numpy_and_tensor_inputs_agree():
    from gpzoo.utilities import dims_autocorr
    X, smooth, noise = _field(4000, 3)
    F = np.stack([smooth, noise, smooth * noise], axis=1)
    a = dims_autocorr(F, X, n_neighs=8)
    b = dims_autocorr(torch.as_tensor(F).cuda(), torch.as_tensor(X).cuda(), n_neighs=8)
    c = dims_autocorr(torch.as_tensor(F), X)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    assert not np.array_equal(a[1], c[1])          # another graph (6 neighbours) ...
    assert a[0].dtype == c[0].dtype == np.int64    # ... same types


def test_dims_autocorr_rejects_bad_inputs():
    from gpzoo.utilities import dims_autocorr
    X, smooth, _ = _field(100, 4)
    F = smooth[:, None]
    with pytest.raises(ValueError, match="n_neighs"):
        dims_autocorr(F[:6], X[:6])
    with pytest.raises(ValueError, match="rows"):
        dims_autocorr(F[:99], X)
    with pytest.raises(ValueError, match="dimension 5"):
        dims_autocorr(F, np.random.default_rng(0).random((100, 5)))
    Xn = X.copy()
    Xn[3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        dims_autocorr(F, Xn)
    Xn[3, 1] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        dims_autocorr(F, Xn)
