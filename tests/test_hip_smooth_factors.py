"""GPU: the exact K-nearest mean (gpz_knn_mean) selects the brute-force oracle's index sets bit for bit -- random points,
exact ties, K = N, M > N, N = 200 000 -- its means match the fp64 oracle and are bitwise reproducible, the C entry
refuses bad arguments without a launch, and smooth_spatial_factors reproduces the reference goldens."""
import functools
import os

import numpy as np
import pytest
import torch

import smooth_oracle as O
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES64 = ["1037x100_d2_L4_f64", "300x150_d1_L3_f64", "300x7_d3_L5_f64", "40x64_d2_L3_f64", "collinear_500x40_d2_L3_f64"]
CASES32 = ["1037x100_d2_L4_f32", "4099x33_d4_L64_f32"]


def golden(name):
    return np.load(os.path.join(GOLDEN, f"extra_smooth_{name}.npz"))


def _knn_mean(X, F, Z, K):
    from gpzoo_amd import ops
    U, idx = ops.knn_mean(torch.as_tensor(X).cuda(), torch.as_tensor(F).cuda(), torch.as_tensor(Z).cuda(), K,
                          return_index=True)
    assert U.dtype == torch.float64 and U.shape == (len(Z), F.shape[1])
    assert idx.dtype == torch.int64 and idx.shape == (len(Z), K)
    return U.cpu().numpy(), idx.cpu().numpy()


def _points(N, d, seed):
    rng = np.random.default_rng(seed)
    return rng.random((N, d)) * 10.0 - 5.0


def _factors(N, L, seed):
    """Factors in [1, 2): every mean is a sum of same-sign terms, so a relative tolerance of a few fp64 roundings is
    meaningful for every entry (a mean that cancels to near zero would have no relative accuracy in ANY summation order)."""
    return np.random.default_rng(seed).random((N, L)) + 1.0


@pytest.mark.parametrize("N,M,d,K,dtype", [
    (7, 3, 2, 2, np.float32), (2, 1, 1, 2, np.float64), (65, 5, 4, 64, np.float64), (257, 300, 1, 2, np.float64),
    (300, 1, 3, 300, np.float32), (1037, 100, 2, 11, np.float32), (4099, 33, 4, 125, np.float64),
    (4099, 64, 3, 1000, np.float32), (70001, 257, 2, 273, np.float32),
])
def test_index_sets_equal_the_oracle(N, M, d, K, dtype):
    X = _points(N, d, N + 7 * d + K).astype(dtype)
    Z = _points(M, d, N + M + 1).astype(dtype)
    F = _factors(N, 2, 3).astype(np.float32)
    U, idx = _knn_mean(X, F, Z, K)
    rows = np.arange(M) if N <= 4099 else np.random.default_rng(1).choice(M, 64, replace=False)
    want_U, want = O.knn_mean(X, F, Z, K, rows)
    np.testing.assert_array_equal(idx[rows], want)
    np.testing.assert_allclose(U[rows], want_U, rtol=1e-12, atol=0)
    assert (np.diff(idx, axis=1) > 0).all() and idx.min() >= 0 and idx.max() < N
    if K == N:
        np.testing.assert_array_equal(idx, np.arange(N)[None])


@functools.lru_cache(maxsize=None)
def _lattice():
    g = np.arange(64, dtype=np.float64)
    X = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    X = X[np.random.default_rng(3).permutation(len(X))]          # index order unrelated to position
    return X, X[::89].copy()                                     # 47 queries ON lattice points


@pytest.mark.parametrize("K", [2, 5, 98])
def test_lattice_ties_go_to_the_lower_index(K):
    """K = 5 cuts the first ring of four equidistant neighbours, K = 2 and 98 cut later rings."""
    X, Z = _lattice()
    F = _factors(len(X), 3, 4)
    U, idx = _knn_mean(X.astype(np.float32), F, Z.astype(np.float32), K)
    want_U, want = O.knn_mean(X, F, Z, K)
    np.testing.assert_array_equal(idx, want)
    np.testing.assert_allclose(U, want_U, rtol=1e-12, atol=0)
    d2 = np.sort(((X[None] - Z[:, None]) ** 2).sum(-1), axis=1)
    assert (d2[:, K - 1] == d2[:, K]).any()                      # the K-th place IS tied for some query


@pytest.mark.parametrize("K", [2, 4, 300])
def test_triplicated_points(K):
    base = _points(700, 2, 5)
    X = np.concatenate([base, base, base])[np.random.default_rng(4).permutation(2100)]
    Z = base[:50]
    F = _factors(2100, 2, 6)
    U, idx = _knn_mean(X, F, Z, K)
    want_U, want = O.knn_mean(X, F, Z, K)
    np.testing.assert_array_equal(idx, want)
    np.testing.assert_allclose(U, want_U, rtol=1e-12, atol=0)
    if K == 2:                                                   # two of the three copies: the two lowest indices
        copies = np.stack([np.nonzero((X == z).all(axis=1))[0][:2] for z in Z])
        np.testing.assert_array_equal(idx, copies)


@pytest.mark.parametrize("K", [1, 7, 257, 300])
def test_identical_points_take_the_lowest_indices(K):
    X = np.full((300, 3), 1.25)
    F = _factors(300, 5, 7)
    U, idx = _knn_mean(X, F, X[:3], K)
    np.testing.assert_array_equal(idx, np.tile(np.arange(K), [3, 1]))
    np.testing.assert_allclose(U, np.tile(F[:K].mean(axis=0), [3, 1]), rtol=1e-12, atol=0)


@functools.lru_cache(maxsize=None)
def _value_sets():
    X, Z = _points(1037, 2, 21), _points(37, 2, 22)
    return X, Z, O.knn_sets(X, Z, 300)


@pytest.mark.parametrize("L", [1, 4, 64, 65, 256])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_means_match_the_oracle_and_are_reproducible(L, dtype):
    """K = 300 of N = 1037: every query's set spans several 256-spot chunks, L on both sides of every column-tile width."""
    X, Z, sets = _value_sets()
    F = _factors(1037, L, L).astype(dtype)
    U1, idx1 = _knn_mean(X, F, Z, 300)
    U2, idx2 = _knn_mean(X, F, Z, 300)
    np.testing.assert_array_equal(idx1, sets)
    np.testing.assert_allclose(U1, F.astype(np.float64)[sets].mean(axis=1), rtol=1e-12, atol=0)
    assert np.array_equal(U1, U2) and np.array_equal(idx1, idx2)                # bit for bit
    assert (np.diff(idx1, axis=1) > 0).all() and idx1.min() >= 0 and idx1.max() < 1037
    from gpzoo_amd import ops
    U3 = ops.knn_mean(torch.as_tensor(X).cuda(), torch.as_tensor(F).cuda(), torch.as_tensor(Z).cuda(), 300)
    assert np.array_equal(U3.cpu().numpy(), U1)                                  # without the index table too


def test_ops_knn_mean_rejects_bad_arguments():
    from gpzoo_amd import ops
    X, F, Z = torch.zeros(10, 2).cuda(), torch.zeros(10, 3).cuda(), torch.zeros(4, 2).cuda()
    for args in ((X[:, 0], F, Z, 2), (X, F[:, 0], Z, 2), (X, F, Z[0], 2), (X, F[:9], Z, 2), (X, F, Z[:, :1], 2),
                 (X, F, Z, 0), (X, F, Z, 11)):
        with pytest.raises(ValueError, match="knn_mean"):
            ops.knn_mean(*args)
    with pytest.raises(ValueError, match="gpz_knn_mean"):
        ops.knn_mean(torch.zeros(10, 5).cuda(), F, torch.zeros(4, 5).cuda(), 2)


@pytest.mark.parametrize("case", CASES64)
def test_smooth_spatial_factors_equals_the_reference_fp64(case):
    from gpzoo.utilities import smooth_spatial_factors
    z = golden(case)
    got = smooth_spatial_factors(z["F"], z["Z"], z["X"])
    for name, g in zip(("U", "beta0", "beta"), got):
        assert isinstance(g, np.ndarray) and g.dtype == np.float64 and g.shape == z[name].shape
        atol = 1e-12 * np.abs(z[name]).max() if case.startswith("collinear") else 0.0
        np.testing.assert_allclose(g, z[name], rtol=1e-10, atol=atol, err_msg=name)


@pytest.mark.parametrize("case", CASES32)
def test_smooth_spatial_factors_equals_the_reference_fp32(case):
    """float32 data: computed in fp64 and rounded once, so it equals the reference run on the float64 cast of the same
    values to one fp32 rounding, and is no further from that fp64 result than the reference's own float32 run."""
    from gpzoo.utilities import smooth_spatial_factors
    z = golden(case)
    got = smooth_spatial_factors(z["F"], z["Z"], z["X"])
    for name, g in zip(("U", "beta0", "beta"), got):
        ref32, ref64 = z[name], z[name + "64"]
        assert isinstance(g, np.ndarray) and g.dtype == np.float32 and g.shape == ref32.shape
        scale = np.abs(ref64).max()
        np.testing.assert_allclose(g, ref64.astype(np.float32), rtol=2e-7, atol=2e-7 * scale, err_msg=name)
        ours, theirs = np.abs(g.astype(np.float64) - ref64).max(), np.abs(ref32.astype(np.float64) - ref64).max()
        print(f"{case} {name}: max|ours - ref64| {ours:.3e}, max|ref32 - ref64| {theirs:.3e}, scale {scale:.3e}")
        assert ours <= theirs + float(np.spacing(np.float32(scale))), name


def test_smooth_spatial_factors_input_kinds_agree():
    from gpzoo.utilities import smooth_spatial_factors
    z = golden("1037x100_d2_L4_f32")
    F, Z, X = z["F"], z["Z"], z["X"]
    a = smooth_spatial_factors(F, Z, X)
    b = smooth_spatial_factors(torch.as_tensor(F).cuda(), torch.as_tensor(Z).cuda(), torch.as_tensor(X).cuda())
    c = smooth_spatial_factors(torch.as_tensor(F), torch.as_tensor(Z), torch.as_tensor(X))
    e = smooth_spatial_factors(torch.as_tensor(F).cuda(), Z, torch.as_tensor(X))
    for u, v, w, x in zip(a, b, c, e):
        assert u.dtype == np.float32
        np.testing.assert_array_equal(u, v)
        np.testing.assert_array_equal(u, w)
        np.testing.assert_array_equal(u, x)
    f = smooth_spatial_factors(F.astype(np.float64), Z, X)                       # float64 factors: float64 outputs
    assert all(v.dtype == np.float64 for v in f)
    np.testing.assert_array_equal(f[0].astype(np.float32), a[0])
    g = smooth_spatial_factors(np.round(F * 4).astype(np.int64), Z, X)           # anything else is taken as float64
    assert all(v.dtype == np.float64 for v in g)


def test_smooth_spatial_factors_with_more_inducing_points_than_spots():
    from gpzoo.utilities import smooth_spatial_factors
    z = golden("40x64_d2_L3_f64")
    assert len(z["Z"]) > len(z["X"]) and int(z["K"]) == 2
    U, _, _ = smooth_spatial_factors(z["F"], z["Z"], z["X"])
    want, _ = O.knn_mean(z["X"], z["F"], z["Z"], 2)
    np.testing.assert_allclose(U, want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("which", ["F", "Z", "X"])
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_smooth_spatial_factors_rejects_non_finite_values(which, value):
    from gpzoo.utilities import smooth_spatial_factors
    z = golden("300x7_d3_L5_f64")
    a = {k: z[k].copy() for k in ("F", "Z", "X")}
    a[which][3, 1] = value
    with pytest.raises(ValueError, match="non-finite"):
        smooth_spatial_factors(a["F"], a["Z"], a["X"])


def test_at_scale():
    """N = 200 000 (a uniform disc plus dense clusters), M = 2 048 spots as inducing points, K = 98, L = 32, float32:
    256 sampled queries against the oracle, every row checked for sanity."""
    rng = np.random.default_rng(11)
    n_disc = 150_000
    r, t = np.sqrt(rng.random(n_disc)) * 100.0, rng.random(n_disc) * 2 * np.pi
    disc = np.stack([r * np.cos(t), r * np.sin(t)], 1)
    centres = rng.random((25, 2)) * 160.0 - 80.0
    clusters = centres[rng.integers(0, 25, 50_000)] + rng.normal(size=(50_000, 2)) * 0.05
    X = np.concatenate([disc, clusters])[rng.permutation(200_000)].astype(np.float32)
    N, M, K, L = len(X), 2048, 98, 32
    Z = X[rng.choice(N, M, replace=False)]
    F = _factors(N, L, 12).astype(np.float32)
    U, idx = _knn_mean(X, F, Z, K)
    rows = rng.choice(M, 256, replace=False)
    want_U, want = O.knn_mean(X, F, Z, K, rows)
    np.testing.assert_array_equal(idx[rows], want)
    np.testing.assert_allclose(U[rows], want_U, rtol=1e-12, atol=0)
    assert np.isfinite(U).all() and U.min() >= 1.0 and U.max() < 2.0
    assert idx.min() >= 0 and idx.max() < N and (np.diff(idx, axis=1) > 0).all()


def test_c_entry_refuses_bad_arguments_without_a_launch():
    from gpzoo_amd import _lib, ops
    lib = _lib.load()
    N, M, d, L, K = 500, 9, 2, 4, 11
    X, Z = torch.rand(N, 4, device="cuda"), torch.rand(M, 4, device="cuda")      # wide enough for the d = 5 probe's d <= 4
    F = torch.rand(N, 257, device="cuda")
    U = torch.full((M, 257), -7.0, dtype=torch.float64, device="cuda")
    idx = torch.full((M, N + 1), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.gpz_knn_mean_workspace_bytes(N, M, 4, N, 256), dtype=torch.uint8, device="cuda")
    ok = dict(X=X, d=d, K=K, L=L, U=U)
    for kw in (dict(d=5), dict(K=0), dict(K=N + 1), dict(L=257), dict(X=None), dict(U=None)):
        a = dict(ok, **kw)
        rc = lib.gpz_knn_mean(ops._ptr(a["X"]), N, ops._ptr(Z), M, a["d"], _lib.GPZ_F32, ops._ptr(F), a["L"], _lib.GPZ_F32,
                              a["K"], ops._ptr(a["U"]), ops._ptr(idx), ops._ptr(ws), ws.numel(), ops._stream(X.device))
        assert rc < 0, kw
        assert b"gpz_knn_mean" in lib.gpz_last_error(), (kw, lib.gpz_last_error())
        if "X" not in kw and "U" not in kw:
            assert lib.gpz_knn_mean_workspace_bytes(N, M, a["d"], a["K"], a["L"]) == 0
            assert b"gpz_knn_mean" in lib.gpz_last_error()
    torch.cuda.synchronize()
    assert bool((U == -7.0).all()) and bool((idx == -7).all())                   # nothing was launched
    assert lib.gpz_knn_mean_workspace_bytes(N, M, d, K, L) > 0
