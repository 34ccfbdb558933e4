"""CPU: the spatial-statistics oracle against sklearn, host-side argument checks of gpz_spatial_knn / gpz_morans_i (no
launch: there is no GPU here) and the public surface of dims_autocorr."""
import ctypes
import inspect

import numpy as np
import pytest

import spatial_oracle as O


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_oracle_matches_sklearn_on_tie_free_data(d, dtype):
    neighbors = pytest.importorskip("sklearn.neighbors")
    rng = np.random.default_rng(10 + d)
    X = rng.random((2000, d)).astype(dtype)
    K = 6
    want = neighbors.NearestNeighbors(n_neighbors=K).fit(X).kneighbors(return_distance=False)
    got = O.knn_rows(X, K)
    assert got.shape == want.shape
    assert all(set(a) == set(b) for a, b in zip(got, want))


def test_oracle_ties_go_to_the_lower_index():
    X = np.array([[0.0, 0.0], [1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0], [0.0, 0.0]])
    assert O.knn_rows(X, 3, rows=[0]).tolist() == [[5, 1, 2]]
    assert O.knn_rows(np.zeros((5, 2)), 2).tolist() == [[1, 2], [0, 2], [0, 1], [0, 1], [0, 1]]


def test_oracle_morans_i():
    V = np.stack([np.arange(6.0), np.full(6, 0.1)], axis=1)
    nbr = np.array([[1], [0], [3], [2], [5], [4]])
    I = O.morans_i(V, nbr)
    z = np.arange(6.0) - 2.5
    assert I[0] == pytest.approx((z * z[nbr[:, 0]]).sum() / (z * z).sum())
    assert np.isnan(I[1])


def _lib():
    from gpzoo_amd import _lib, build
    build.build(force=False, verbose=False)
    return _lib.load()


def test_spatial_knn_rejects_bad_arguments_on_the_host():
    lib = _lib()
    buf = ctypes.c_void_p(16)                 # never dereferenced: every call below fails its host checks first
    ok = dict(X=buf, N=100, d=2, K=6, dtype=0, order=None, idx=buf, ws=buf, ws_bytes=1 << 30, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gpz_spatial_knn(a["X"], a["N"], a["d"], a["K"], a["dtype"], a["order"], a["idx"], a["ws"],
                                   a["ws_bytes"], a["stream"])

    for kw, msg in [(dict(X=None), b"null"), (dict(idx=None), b"null"), (dict(ws=None), b"null"),
                    (dict(K=0), b"K=0"), (dict(K=33), b"K=33"), (dict(d=0), b"d=0"), (dict(d=5), b"d=5"),
                    (dict(N=6), b"N=6"), (dict(N=3, K=6), b"N=3"), (dict(N=1 << 31), b"N="), (dict(dtype=2), b"dtype"),
                    (dict(ws_bytes=16), b"workspace")]:
        assert call(**kw) < 0, kw
        assert msg in lib.gpz_last_error(), (kw, lib.gpz_last_error())
    assert lib.gpz_spatial_knn_workspace_bytes(100, 2, 6) >= 100 * 36
    assert lib.gpz_spatial_knn_workspace_bytes(6, 2, 6) == 0
    assert lib.gpz_spatial_knn_workspace_bytes(100, 5, 6) == 0
    assert lib.gpz_spatial_knn_workspace_bytes(100, 2, 33) == 0


def test_morans_i_rejects_bad_arguments_on_the_host():
    lib = _lib()
    buf = ctypes.c_void_p(16)
    ok = dict(V=buf, N=100, L=3, dtype=1, nbr=buf, K=6, I=buf, info=buf, ws=buf, ws_bytes=1 << 30, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gpz_morans_i(a["V"], a["N"], a["L"], a["dtype"], a["nbr"], a["K"], a["I"], a["info"], a["ws"],
                                a["ws_bytes"], a["stream"])

    for kw, msg in [(dict(V=None), b"null"), (dict(nbr=None), b"null"), (dict(I=None), b"null"),
                    (dict(info=None), b"null"), (dict(ws=None), b"null"), (dict(dtype=3), b"dtype"),
                    (dict(K=0), b"K=0"), (dict(N=6), b"N=6"), (dict(L=0), b"L=0"), (dict(ws_bytes=16), b"workspace")]:
        assert call(**kw) < 0, kw
        assert msg in lib.gpz_last_error(), (kw, lib.gpz_last_error())
    assert lib.gpz_morans_i_workspace_bytes(100, 3, 6) > 0
    assert lib.gpz_morans_i_workspace_bytes(100, 0, 6) == 0


def test_dims_autocorr_resolves_with_the_reference_signature():
    from gpzoo.utilities import dims_autocorr
    import gpzoo_amd.utilities as U
    assert dims_autocorr is U.dims_autocorr
    assert "dims_autocorr" not in U._NOT_REBUILT
    params = inspect.signature(dims_autocorr).parameters
    assert list(params)[:3] == ["factors", "coords", "sort"] and params["sort"].default is True
    assert params["n_neighs"].kind is inspect.Parameter.KEYWORD_ONLY and params["n_neighs"].default == 6
