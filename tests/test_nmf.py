"""CPU: the NMF oracle against sklearn (exact in fp64), nmf.initialize_nmf against sklearn's _initialize_nmf, the
precomputed path of regularized_nmf against the goldens, host-side argument checks of the gpz_nmf_kl_* entries (no
launch: there is no GPU here) and the public surface."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

import nmf_oracle as O
from conftest import GOLDEN

CASES = ["nndsvdar_600x150", "nndsvda_1037x80_tol0", "nndsvd_600x150_sz", "random_600x150"]


def golden(name):
    z = np.load(os.path.join(GOLDEN, f"extra_nmf_{name}.npz"))
    return z, json.loads(str(z["kwargs"]))


def _start(N, D, L, seed):
    rng = np.random.default_rng(seed)
    return np.abs(rng.standard_normal((N, L))) + 0.1, np.abs(rng.standard_normal((L, D))) + 0.1


@pytest.mark.parametrize("N,D,L", [(63, 17, 3), (257, 130, 5), (600, 150, 4)])
@pytest.mark.parametrize("tol", [0.0, 1e-4])
def test_oracle_equals_sklearn_bit_for_bit(N, D, L, tol):
    from sklearn.decomposition._nmf import _beta_divergence, _fit_multiplicative_update
    X = O.planted_counts(N, D, L, 100 + N)
    X[3] = 0.0                                      # an empty row and an empty column
    X[:, 5] = 0.0
    W0, H0 = _start(N, D, L, N)
    assert O.kl_divergence(X, W0, H0) == _beta_divergence(X, W0, H0, 1, square_root=True)
    W, H, n_iter = O.fit_mu(X, W0, H0, max_iter=60, tol=tol)
    Ws, Hs, n_s = _fit_multiplicative_update(X, W0.copy(), H0.copy(), "kullback-leibler", max_iter=60, tol=tol)
    assert n_iter == n_s and (tol > 0 or n_iter == 60)
    np.testing.assert_array_equal(W, Ws)
    np.testing.assert_array_equal(H, Hs)
    assert O.kl_divergence(X, W, H) == _beta_divergence(X, Ws, Hs, 1, square_root=True)


def test_oracle_leaves_its_starting_values_alone():
    X = O.planted_counts(40, 30, 3, 1)
    W0, H0 = _start(40, 30, 3, 2)
    keep = W0.copy(), H0.copy()
    O.fit_mu(X, W0, H0, max_iter=3, tol=0)
    np.testing.assert_array_equal(W0, keep[0])
    np.testing.assert_array_equal(H0, keep[1])


@pytest.mark.parametrize("case", ["nndsvdar_600x150", "nndsvda_1037x80_tol0", "nndsvd_600x150_sz"])
@pytest.mark.parametrize("init", ["nndsvd", "nndsvda", "nndsvdar", None])
def test_initialize_nmf_matches_sklearn(case, init):
    """On fixtures whose triplets are converged (the generator's conditions (a) and (b)): the same zeros, values within
    1e-7 absolute -- ten times the fixture condition, far below the 1e-6 clipping threshold and the avg / 100 scale of
    the random fill."""
    from sklearn.decomposition._nmf import _initialize_nmf
    from gpzoo_amd import nmf
    z, kw = golden(case)
    Y, L = z["Y"].astype(np.float64), int(z["L"])
    Ws, Hs = _initialize_nmf(Y, L, init=init, random_state=kw["random_state"])
    W, H = nmf.initialize_nmf(torch.as_tensor(Y), L, init=init, random_state=kw["random_state"])
    assert W.dtype == torch.float64 and W.shape == Ws.shape and H.shape == Hs.shape
    W, H = W.numpy(), H.numpy()
    np.testing.assert_array_equal(W == 0, Ws == 0)
    np.testing.assert_array_equal(H == 0, Hs == 0)
    assert np.abs(W - Ws).max() <= 1e-7 and np.abs(H - Hs).max() <= 1e-7
    if init == kw["init"]:                          # and the starting values the golden run used
        assert np.abs(W - z["W0"]).max() <= 1e-7 and np.abs(H - z["H0"]).max() <= 1e-7


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_initialize_nmf_random_is_exact(dtype):
    from sklearn.decomposition._nmf import _initialize_nmf
    from gpzoo_amd import nmf
    z, _ = golden("random_600x150")
    Y = z["Y"].astype(dtype)
    for L, seed in ((4, 5), (700, 0)):              # L > min(N, D): allowed for 'random', and what None then selects
        Ws, Hs = _initialize_nmf(Y, L, init="random", random_state=seed)
        W, H = nmf.initialize_nmf(torch.as_tensor(Y), L, init="random" if L == 4 else None, random_state=seed)
        assert W.numpy().dtype == dtype
        np.testing.assert_array_equal(W.numpy(), Ws)
        np.testing.assert_array_equal(H.numpy(), Hs)
        if L == 4 and dtype is np.float64:          # the golden run's own starting values
            np.testing.assert_array_equal(W.numpy(), z["W0"])
            np.testing.assert_array_equal(H.numpy(), z["H0"])


def test_initialize_nmf_rejects_bad_arguments():
    from gpzoo_amd import nmf
    Y = torch.ones(8, 5, dtype=torch.float64)
    with pytest.raises(ValueError, match="n_components <= min"):
        nmf.initialize_nmf(Y, 6, init="nndsvd")
    with pytest.raises(ValueError, match="unsupported"):
        nmf.initialize_nmf(Y, 2, init="custom")
    with pytest.raises(ValueError):
        nmf.initialize_nmf(Y[0], 2)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("tag", ["64", "32"])
def test_precomputed_path_equals_the_golden_postprocessing(case, tag):
    from gpzoo.utilities import regularized_nmf
    z, _ = golden(case)
    L, shrinkage = int(z["L"]), float(z["shrinkage"])
    sz = z["sz"] if z["sz"].ndim else 1
    eF, Wl = z["nmfW" + tag].copy(), z["nmfH" + tag].T     # components_.T: a view, as the reference passes it on (float32 sums depend on the memory order)
    keep = eF.copy(), Wl.copy()
    F, W = regularized_nmf(None, L, sz=sz, factors=eF, loadings=Wl, shrinkage=shrinkage)
    assert F.dtype == z["F" + tag].dtype and W.dtype == z["W" + tag].dtype
    assert F.shape == z["F" + tag].shape and W.shape == z["W" + tag].shape
    rtol = 1e-12 if tag == "64" else 0.0             # the float32 arithmetic is the same numpy expression: exact
    np.testing.assert_allclose(F, z["F" + tag], rtol=rtol, atol=0)
    np.testing.assert_allclose(W, z["W" + tag], rtol=rtol, atol=0)
    np.testing.assert_array_equal(eF, keep[0])
    np.testing.assert_array_equal(Wl, keep[1])
    if tag == "64":                                 # the oracle's post-processing is the same function
        Fo, Wo = O.postprocess(eF, Wl, L, sz=sz, shrinkage=shrinkage)
        np.testing.assert_allclose(Fo, F, rtol=1e-12, atol=0)
        np.testing.assert_allclose(Wo, W, rtol=1e-12, atol=0)


@pytest.mark.parametrize("shrinkage", [0.0, 1.0])
def test_precomputed_path_never_modifies_its_inputs(shrinkage):
    """Outside (0, 1) nothing is shrunk and the reference scales the caller's loadings in place; here it does not."""
    from gpzoo.utilities import regularized_nmf
    z, _ = golden("random_600x150")
    eF, Wl = z["nmfW64"].copy(), np.ascontiguousarray(z["nmfH64"].T)
    keep = eF.copy(), Wl.copy()
    F, W = regularized_nmf(None, 4, factors=eF, loadings=Wl, shrinkage=shrinkage)
    np.testing.assert_array_equal(eF, keep[0])
    np.testing.assert_array_equal(Wl, keep[1])
    Fo, Wo = O.postprocess(eF, Wl, 4, shrinkage=shrinkage)
    np.testing.assert_allclose(F, Fo, rtol=1e-12)
    np.testing.assert_allclose(W, Wo, rtol=1e-12)


def _lib():
    from gpzoo_amd import _lib, build
    build.build(force=False, verbose=False)
    return _lib.load()


def test_nmf_entries_reject_bad_arguments_on_the_host():
    lib = _lib()
    buf = ctypes.c_void_p(16)                 # never dereferenced: every call below fails its host checks first
    ok = dict(X=buf, W=buf, H=buf, N=100, D=50, L=4, dtype=0, iters=1, out=buf, ws=buf, ws_bytes=1 << 30, stream=None)

    def update(**kw):
        a = dict(ok, **kw)
        return lib.gpz_nmf_kl_update(a["X"], a["W"], a["H"], a["N"], a["D"], a["L"], a["dtype"], a["iters"], a["ws"],
                                     a["ws_bytes"], a["stream"])

    def divergence(**kw):
        a = dict(ok, **kw)
        return lib.gpz_nmf_kl_divergence(a["X"], a["W"], a["H"], a["N"], a["D"], a["L"], a["dtype"], a["out"], a["ws"],
                                         a["ws_bytes"], a["stream"])

    bad = [(dict(X=None), b"null"), (dict(W=None), b"null"), (dict(H=None), b"null"), (dict(ws=None), b"null"),
           (dict(L=0), b"L=0"), (dict(L=65), b"L=65"), (dict(dtype=2), b"dtype"), (dict(N=0), b"N=0"), (dict(D=0), b"D=0"),
           (dict(N=1 << 31), b"N="), (dict(N=1 << 21, D=1 << 20), b"N="), (dict(ws_bytes=16), b"workspace")]
    for fn, more in ((update, [(dict(iters=0), b"iters=0")]), (divergence, [(dict(out=None), b"null")])):
        for kw, msg in bad + more:
            assert fn(**kw) < 0, kw
            assert msg in lib.gpz_last_error(), (kw, lib.gpz_last_error())
    assert lib.gpz_nmf_kl_workspace_bytes(100, 50, 4, 0) > 0
    assert lib.gpz_nmf_kl_workspace_bytes(100, 50, 4, 1) >= lib.gpz_nmf_kl_workspace_bytes(100, 50, 4, 0)
    for N, D, L, dt in ((100, 50, 0, 0), (100, 50, 65, 0), (100, 50, 4, 2), (0, 50, 4, 0), (100, 0, 4, 1),
                        (1 << 21, 1 << 20, 4, 0)):
        assert lib.gpz_nmf_kl_workspace_bytes(N, D, L, dt) == 0
        assert b"gpz_nmf_kl_workspace_bytes" in lib.gpz_last_error()


def test_names_resolve_with_the_reference_signatures():
    import gpzoo.utilities as G
    import gpzoo_amd.utilities as U
    for name in ("regularized_nmf", "shrink_factors", "shrink_loadings", "lnormal_approx_dirichlet"):
        assert getattr(G, name) is getattr(U, name)
        assert name not in U._NOT_REBUILT
    p = inspect.signature(U.regularized_nmf).parameters
    assert list(p) == ["Y", "L", "sz", "pseudocount", "factors", "loadings", "shrinkage", "kwargs"]
    assert (p["sz"].default, p["pseudocount"].default, p["factors"].default, p["loadings"].default,
            p["shrinkage"].default) == (1, 1e-2, None, None, 0.2)
    assert p["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    for fn, first in ((U.shrink_factors, "F"), (U.shrink_loadings, "W")):
        q = inspect.signature(fn).parameters
        assert list(q) == [first, "shrinkage"] and q["shrinkage"].default == 0.2
    assert list(inspect.signature(U.lnormal_approx_dirichlet).parameters) == ["L"]


def test_helpers_follow_their_formulas():
    from gpzoo.utilities import lnormal_approx_dirichlet, shrink_factors, shrink_loadings
    assert lnormal_approx_dirichlet(1) == (0.0, 0.0)
    mu, sigma = lnormal_approx_dirichlet(20)
    assert sigma ** 2 == pytest.approx(np.log(40 / 21)) and mu == pytest.approx(-np.log(20) - np.log(40 / 21) / 2)
    A = np.random.default_rng(0).random((7, 3))
    F = shrink_factors(A, 0.3)
    np.testing.assert_allclose(F.sum(axis=1), A.sum(axis=1))
    np.testing.assert_allclose(F, 0.7 * A + 0.3 * A.mean(axis=1, keepdims=True))
    W = shrink_loadings(A, 0.3)
    np.testing.assert_allclose(W.sum(axis=0), A.sum(axis=0))
    np.testing.assert_allclose(W, 0.7 * A + 0.3 * A.mean(axis=0))
    assert shrink_factors(A, 0.0) is A and shrink_loadings(A, 1.0) is A


@pytest.mark.parametrize("kw,word", [
    (dict(), "solver"), (dict(solver="cd", beta_loss="kullback-leibler"), "solver"),
    (dict(solver="mu"), "beta_loss"), (dict(solver="mu", beta_loss="frobenius"), "beta_loss"),
    (dict(solver="mu", beta_loss="itakura-saito"), "beta_loss"), (dict(solver="mu", beta_loss=2), "beta_loss"),
    (dict(solver="mu", beta_loss=1, alpha_W=0.1), "alpha_W"), (dict(solver="mu", beta_loss=1, alpha_H=0.5), "alpha_H"),
    (dict(solver="mu", beta_loss=1, init="custom"), "init"), (dict(solver="mu", beta_loss=1, n_components=3), "n_components"),
    (dict(solver="mu", beta_loss="kullback-leibler", batch_size=10), "batch_size"),
])
def test_unsupported_keywords_raise_before_any_gpu_use(kw, word, monkeypatch):
    from gpzoo.utilities import regularized_nmf

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the keywords were checked")

    monkeypatch.setattr(torch.cuda, "current_device", no_gpu)
    monkeypatch.setattr(torch.Tensor, "to", no_gpu)
    with pytest.raises(NotImplementedError, match=word):
        regularized_nmf(np.ones((6, 5)), 2, **kw)
