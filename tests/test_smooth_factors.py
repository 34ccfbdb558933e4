"""CPU: the host helpers of the NSF initialisation chain (rescale_spatial_coords, init_softplus, scanpy_sizefactors)
and the X=None branch of smooth_spatial_factors against the reference goldens, the argument checks that come before any
GPU use, the public surface, and the brute-force oracle against every golden U (no launch: there is no GPU here)."""
import inspect
import os

import numpy as np
import pytest
import torch

import smooth_oracle as O
from conftest import GOLDEN, ROOT

CASES = ["1037x100_d2_L4_f64", "1037x100_d2_L4_f32", "300x150_d1_L3_f64", "300x7_d3_L5_f64", "4099x33_d4_L64_f32",
         "40x64_d2_L3_f64", "collinear_500x40_d2_L3_f64"]
NAMES = ("smooth_spatial_factors", "rescale_spatial_coords", "init_softplus", "scanpy_sizefactors")


def golden(name):
    return np.load(os.path.join(GOLDEN, f"extra_smooth_{name}.npz"))


def _rtol(tag):
    return 1e-12 if tag == "64" else 1e-6


@pytest.mark.parametrize("tag", ["64", "32"])
def test_rescale_spatial_coords_matches_the_golden_and_leaves_its_argument_alone(tag):
    from gpzoo.utilities import rescale_spatial_coords
    z = golden("helpers")
    X = z["coords" + tag].copy()
    for out, kw in ((z["rescaled" + tag], {}), (z["rescaled6_" + tag], dict(box_side=6))):
        got = rescale_spatial_coords(X, **kw)
        assert got.dtype == out.dtype and got.shape == out.shape
        np.testing.assert_allclose(got, out, rtol=_rtol(tag), atol=_rtol(tag) * np.abs(out).max())
        np.testing.assert_array_equal(X, z["coords" + tag])          # (the reference shifts and scales it in place)
    if tag == "64":
        np.testing.assert_allclose(rescale_spatial_coords(z["coords3d"]), z["rescaled3d"], rtol=1e-12,
                                   atol=1e-12 * np.abs(z["rescaled3d"]).max())
    got = rescale_spatial_coords(X)
    assert abs(got.mean(axis=0)).max() < 1e-5
    extent = got.max(axis=0) - got.min(axis=0)
    assert np.prod(extent.astype(np.float64)) == pytest.approx(16.0, rel=1e-5)     # box_side ** d


@pytest.mark.parametrize("tag", ["64", "32"])
def test_init_softplus_matches_the_golden(tag):
    from gpzoo.utilities import init_softplus
    z = golden("helpers")
    mat = z["mat" + tag].copy()
    assert (mat < 20).any() and (mat >= 20).any()
    for out, kw in ((z["softplus" + tag], {}), (z["softplus_min" + tag], dict(minval=1e-3))):
        got = init_softplus(mat, **kw)
        assert got.dtype == out.dtype
        np.testing.assert_allclose(got, out, rtol=_rtol(tag), atol=0)
        np.testing.assert_array_equal(mat, z["mat" + tag])
    got = init_softplus(mat)
    np.testing.assert_array_equal(got[mat >= 20], mat[mat >= 20])
    # softplus of the result gives the matrix back: log(exp(x) + minval) is within minval = 1e-5 of x
    np.testing.assert_allclose(np.log1p(np.exp(got.astype(np.float64))), mat.astype(np.float64), rtol=0, atol=1e-4)


@pytest.mark.parametrize("tag", ["64", "32"])
def test_scanpy_sizefactors_matches_the_golden(tag):
    from gpzoo.utilities import scanpy_sizefactors
    z = golden("helpers")
    got = scanpy_sizefactors(z["counts" + tag])
    assert got.dtype == z["sizefactors" + tag].dtype and got.shape == (60, 1)
    np.testing.assert_allclose(got, z["sizefactors" + tag], rtol=_rtol(tag), atol=0)
    assert np.median(got) == pytest.approx(1.0)


@pytest.mark.parametrize("tag", ["64", "32"])
@pytest.mark.parametrize("kind", ["numpy", "tensor"])
def test_no_coordinates_branch_matches_the_golden_without_a_gpu(tag, kind, monkeypatch):
    from gpzoo.utilities import smooth_spatial_factors
    from gpzoo_amd import _lib

    def no_gpu(*a, **k):
        raise AssertionError("X=None must not touch the GPU or load the library")

    monkeypatch.setattr(torch.cuda, "current_device", no_gpu)
    monkeypatch.setattr(torch.Tensor, "to", no_gpu)
    monkeypatch.setattr(_lib, "load", no_gpu)
    z = golden("xnone")
    F = z["F"].astype(np.float64 if tag == "64" else np.float32)
    Z = z["Z"]
    if kind == "tensor":
        F, Z = torch.as_tensor(F), torch.as_tensor(Z)
    U, beta0, beta = smooth_spatial_factors(F, Z)
    assert beta is None
    assert isinstance(U, np.ndarray) and isinstance(beta0, np.ndarray)
    assert U.dtype == beta0.dtype == z["U" + tag].dtype and U.shape == (9, 6) and beta0.shape == (6,)
    np.testing.assert_allclose(U, z["U" + tag], rtol=_rtol(tag), atol=0)
    np.testing.assert_allclose(beta0, z["beta0" + tag], rtol=_rtol(tag), atol=0)
    np.testing.assert_array_equal(U, np.tile(beta0, [9, 1]))


def _bad_calls():
    rng = np.random.default_rng(0)
    F, Z, X = rng.random((50, 3)), rng.random((7, 2)), rng.random((50, 2))
    return [
        ((F[:, 0], Z, X), "F must be"), ((F[None], Z, X), "F must be"), ((F[:, 0], Z, None), "F must be"),
        ((F, Z[0], X), "Z must be"), ((F, Z[0], None), "Z must be"), ((F, Z, X[:, 0]), "X must be"),
        ((F, Z, X[:49]), "rows"), ((F[:49], Z, X), "rows"),
        ((F, rng.random((7, 3)), X), "coordinates per point"),
        ((F, rng.random((7, 5)), rng.random((50, 5))), "dimension 5"),
        ((F, rng.random((7, 0)), rng.random((50, 0))), "dimension 0"),
        ((rng.random((50, 257)), Z, X), "L=257"), ((rng.random((50, 0)), Z, X), "L=0"),
        ((F, rng.random((0, 2)), X), "no inducing point"),
        ((F[:1], Z, X[:1]), "n_neighbors=2"),
    ]


@pytest.mark.parametrize("args,word", _bad_calls())
@pytest.mark.parametrize("kind", ["numpy", "tensor"])
def test_bad_arguments_raise_before_any_gpu_use(args, word, kind, monkeypatch):
    from gpzoo.utilities import smooth_spatial_factors
    from gpzoo_amd import _lib

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the arguments were checked")

    monkeypatch.setattr(torch.cuda, "current_device", no_gpu)
    monkeypatch.setattr(torch.Tensor, "to", no_gpu)
    monkeypatch.setattr(_lib, "load", no_gpu)
    if kind == "tensor":
        args = tuple(a if a is None else torch.as_tensor(a) for a in args)
    with pytest.raises(ValueError, match=word):
        smooth_spatial_factors(*args)


def test_names_resolve_with_the_reference_signatures():
    import gpzoo.utilities as G
    import gpzoo_amd.utilities as U
    for name in NAMES:
        assert name not in U._NOT_REBUILT
        assert getattr(G, name) is getattr(U, name)
        assert inspect.isfunction(getattr(U, name)) and getattr(U, name).__doc__
    for name in ("build_group_distances", "anndata_to_train_val", "plot_factors"):
        assert name in U._NOT_REBUILT

    def sig(fn):
        return [(n, p.default) for n, p in inspect.signature(fn).parameters.items()]

    E = inspect.Parameter.empty
    assert sig(U.smooth_spatial_factors) == [("F", E), ("Z", E), ("X", None)]
    assert sig(U.rescale_spatial_coords) == [("X", E), ("box_side", 4)]
    assert sig(U.init_softplus) == [("mat", E), ("minval", 1e-5)]
    assert sig(U.scanpy_sizefactors) == [("Y", E)]


def test_the_chain_runs_without_sklearn_being_imported_by_the_package():
    """The four functions are plain numpy / torch: importing the package and calling the host ones pulls in no sklearn
    (run in a fresh interpreter: this process has imported it for other tests)."""
    import subprocess
    import sys
    code = ("import sys, numpy as np\n"
            "from gpzoo.utilities import smooth_spatial_factors, rescale_spatial_coords, init_softplus, scanpy_sizefactors\n"
            "X = rescale_spatial_coords(np.random.default_rng(0).random((30, 2)))\n"
            "init_softplus(X + 3.0); scanpy_sizefactors(X + 3.0); smooth_spatial_factors(X, X[:4])\n"
            "assert not any(m == 'sklearn' or m.startswith('sklearn.') for m in sys.modules)\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT, timeout=300)


def test_knn_mean_symbols_are_bound_and_declared():
    from gpzoo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpzoo_hip.h")).read()
    for name in ("gpz_knn_mean", "gpz_knn_mean_workspace_bytes"):
        assert name in _lib.exported_symbols()
        assert f"{name}(" in hdr
    assert "#define GPZ_VERSION 212" in hdr


def test_ops_knn_mean_needs_cuda_tensors():
    from gpzoo_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.knn_mean(torch.zeros(5, 2), torch.zeros(5, 1), torch.zeros(2, 2), 2)


def _lib_built():
    from gpzoo_amd import _lib, build
    build.build(force=False, verbose=False)
    return _lib.load()


def test_knn_mean_entry_rejects_bad_arguments_on_the_host():
    """Host checks only (no launch: every call fails them): the same refusals run on the GPU in test_hip_smooth_factors."""
    import ctypes
    lib = _lib_built()
    buf = ctypes.c_void_p(16)                 # never dereferenced
    ok = dict(X=buf, N=100, Z=buf, M=7, d=2, dtype=0, F=buf, L=4, f_dtype=1, K=15, U=buf, idx=None, ws=buf,
              ws_bytes=1 << 30, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gpz_knn_mean(a["X"], a["N"], a["Z"], a["M"], a["d"], a["dtype"], a["F"], a["L"], a["f_dtype"], a["K"],
                                a["U"], a["idx"], a["ws"], a["ws_bytes"], a["stream"])

    bad = [(dict(X=None), b"null"), (dict(Z=None), b"null"), (dict(F=None), b"null"), (dict(U=None), b"null"),
           (dict(ws=None), b"null"), (dict(d=0), b"d=0"), (dict(d=5), b"d=5"), (dict(K=0), b"K=0"), (dict(K=101), b"K=101"),
           (dict(L=0), b"L=0"), (dict(L=257), b"L=257"), (dict(N=0, K=0), b"N=0"), (dict(N=1 << 31), b"N="),
           (dict(M=0), b"M=0"), (dict(dtype=2), b"dtype"), (dict(f_dtype=-1), b"dtype"), (dict(ws_bytes=16), b"workspace")]
    for kw, msg in bad:
        assert call(**kw) < 0, kw
        err = lib.gpz_last_error()
        assert msg in err and b"gpz_knn_mean" in err, (kw, err)
    assert lib.gpz_knn_mean_workspace_bytes(100, 7, 2, 15, 4) >= (100 + 7) * 2 * 8
    for N, M, d, K, L in ((100, 7, 5, 15, 4), (100, 7, 2, 0, 4), (100, 7, 2, 101, 4), (100, 7, 2, 15, 257), (100, 0, 2, 15, 4),
                          (0, 7, 2, 1, 4)):
        assert lib.gpz_knn_mean_workspace_bytes(N, M, d, K, L) == 0
        assert b"gpz_knn_mean_workspace_bytes" in lib.gpz_last_error()


def test_goldens_hold_what_the_gpu_tests_rely_on():
    """Each fixture's K is the reference's rule, and the K-th and (K+1)-th squared distances of every query differ by more
    than 1e-5 relative (the generator's condition (a)): the reference's neighbour choice is unambiguous."""
    for case in CASES:
        z = golden(case)
        X, Z = z["X"].astype(np.float64), z["Z"].astype(np.float64)
        N, M, K = len(X), len(Z), int(z["K"])
        assert K == max(2, -(-N // M))
        d2 = ((X[None] - Z[:, None]) ** 2).sum(-1)
        d2.sort(axis=1)
        assert ((d2[:, K] - d2[:, K - 1]) > 1e-5 * d2[:, K]).all()
        want = np.float32 if case.endswith("f32") else np.float64
        assert z["F"].dtype == z["U"].dtype == z["beta0"].dtype == z["beta"].dtype == want
        assert z["U"].shape == (M, z["F"].shape[1]) and z["beta"].shape == (z["F"].shape[1], X.shape[1])
    z = golden("collinear_500x40_d2_L3_f64")
    assert np.linalg.matrix_rank(z["X"] - z["X"].mean(axis=0)) == 1


@pytest.mark.parametrize("case", CASES)
def test_oracle_reproduces_the_reference_knn_mean(case):
    """The brute-force (d^2, index) restatement equals sklearn's KNeighborsRegressor on every fixture: to fp64 rounding
    of a K-term mean for float64 data; for float32 data against the reference run on the float64 cast of the same values
    (the reference's own float32 result carries its float32 arithmetic)."""
    z = golden(case)
    U, sets = O.knn_mean(z["X"], z["F"], z["Z"], int(z["K"]))
    assert sets.shape == (len(z["Z"]), int(z["K"])) and (np.diff(sets, axis=1) > 0).all()
    if case.endswith("f64"):
        np.testing.assert_allclose(U, z["U"], rtol=1e-12, atol=0)
    else:
        np.testing.assert_allclose(U, z["U64"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(U.astype(np.float32), z["U"], rtol=1e-5, atol=0)
