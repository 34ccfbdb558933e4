"""GPU: kmeans_inducing_points and its three entries (gpz_kmeans_seed / _lloyd / _assign) against the numpy oracle
(tests/kmeans_oracle.py) and the sklearn goldens -- never against the code under test.  Choices (labels, seeding indices,
iteration counts, stop reasons) are compared exactly: d^2 is the same arithmetic bit for bit, and the goldens keep every
choice more than 1e-9 relative from a tie.  Sums (centres, inertia) are compared to 1e-12: the kernels add in fixed trees, the
oracle in ascending index, which moves an fp64 sum of these sizes by a few 1e-16 relative."""
import os

import numpy as np
import pytest
import torch

import kmeans_cases as K
import kmeans_oracle as O
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def golden(name):
    return np.load(os.path.join(GOLDEN, f"extra_kmeans_{name}.npz"))


def cuda(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def one_iteration(X, C0, tol_abs=0.0):
    """One Lloyd iteration through ops: (centres, labels, state record as numpy int64[4])."""
    from gpzoo_amd import ops
    Xd, C = cuda(X), cuda(C0, torch.float64).clone()
    labels = torch.full((len(X),), -1, dtype=torch.int32, device="cuda")
    state = ops.kmeans_state(Xd.device)
    ops.kmeans_lloyd(Xd, C, labels, state, tol_abs, 1)
    return C.cpu().numpy(), labels.cpu().numpy().astype(np.int64), state.cpu().numpy()


def close(got, want, what=""):
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * max(1.0, np.abs(want).max()), err_msg=what)


@pytest.mark.parametrize("case", K.GOLDENS)
def test_goldens(case):
    from gpzoo.utilities import kmeans_inducing_points
    z = golden(case)
    o = O.lloyd(z["X"], z["C0"], int(z["max_iter"]), float(z["tol"]))
    C, info = kmeans_inducing_points(z["X"], len(z["C0"]), init=z["C0"], max_iter=int(z["max_iter"]), tol=float(z["tol"]),
                                     return_info=True)
    assert C.dtype == z["X"].dtype and info["labels"].dtype == np.int64 and info["seed_indices"] is None
    np.testing.assert_array_equal(info["labels"], z["labels"])
    np.testing.assert_array_equal(info["labels"], o["labels"])
    assert info["n_iter"] == int(z["n_iter"]) == o["n_iter"]
    assert info["converged"] == o["converged"]
    if case in K.GOLDEN_STOP:
        assert info["converged"] == K.GOLDEN_STOP[case]
    scale = np.abs(z["centers"]).max()
    if case.endswith("f32"):
        np.testing.assert_allclose(C, z["centers"], rtol=0, atol=1e-5 * scale)
        assert info["inertia"] == pytest.approx(float(z["inertia"]), rel=1e-5)
        np.testing.assert_allclose(C.astype(np.float64), z["centers64"], rtol=0, atol=1e-7 * scale)   # one fp32 rounding
        assert info["inertia"] == pytest.approx(float(z["inertia64"]), rel=1e-12)
    else:
        np.testing.assert_allclose(C, z["centers"], rtol=0, atol=1e-12 * scale)
        np.testing.assert_allclose(C, o["centres"], rtol=0, atol=1e-12 * scale)
        assert info["inertia"] == pytest.approx(float(z["inertia"]), rel=1e-12, abs=1e-12 * scale ** 2)
    assert info["inertia"] == pytest.approx(o["inertia"], rel=1e-12, abs=1e-12 * scale ** 2)


@pytest.mark.parametrize("N,M,d,dtype", K.edge_cases())
def test_edges_one_iteration_and_assign(N, M, d, dtype):
    from gpzoo_amd import ops
    X, C0 = K.random_case(N, M, d, dtype)
    want_C, want_labels, want_shift, moved = O.lloyd_iter(X, C0)
    C, labels, state = one_iteration(X, C0)
    np.testing.assert_array_equal(labels, want_labels)
    close(C, want_C)
    assert state[0] == 1 and state[1] == 0 and state[3] == len(moved)
    assert state[2:3].view(np.float64)[0] == pytest.approx(want_shift, rel=1e-12)
    got, inertia, d2 = ops.kmeans_assign(cuda(X), cuda(C0, torch.float64), return_d2=True)
    np.testing.assert_array_equal(got.cpu().numpy(), want_labels)
    np.testing.assert_array_equal(d2.cpu().numpy(), O.assign(X, C0)[1])                # the same arithmetic: bit for bit
    assert float(inertia) == pytest.approx(O.inertia_of(X, C0, want_labels), rel=1e-12)


@pytest.mark.parametrize("N,M,what", K.PATH_CASES)
def test_assignment_paths(N, M, what):
    from gpzoo_amd import ops
    X, C0 = K.random_case(N, M, 2, "f32", seed=11)
    want, want_d2 = O.assign(X, C0)
    got, inertia, d2 = ops.kmeans_assign(cuda(X), cuda(C0, torch.float64), return_d2=True)
    np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=what)
    np.testing.assert_array_equal(d2.cpu().numpy(), want_d2, err_msg=what)
    assert float(inertia) == pytest.approx(float(want_d2.sum()), rel=1e-12)
    kept, inertia2 = ops.kmeans_assign(cuda(X), cuda(C0, torch.float64), labels=got)    # the inertia of given labels
    assert kept is got and float(inertia2) == float(inertia)


def test_member_sums_of_blobs():
    X, C0, sizes = K.blob_case()
    want_C, want_labels, _, moved = O.lloyd_iter(X, C0)
    C, labels, state = one_iteration(X, C0)
    np.testing.assert_array_equal(labels, want_labels)
    assert np.bincount(labels).tolist() == sizes and not moved and state[3] == 0
    close(C, want_C)
    for k in range(len(sizes)):                                                        # and against a plain fp64 mean
        close(C[k], X[labels == k].mean(axis=0))


@pytest.mark.parametrize("d", [1, 4])
def test_member_sums_all_points_in_one_cluster(d):
    X, _ = K.random_case(1000, 1, d)
    C, labels, _ = one_iteration(X, np.zeros((1, d)))
    assert (labels == 0).all()
    close(C, X.astype(np.float64).mean(axis=0, keepdims=True))


def test_ties_go_to_the_lower_index_and_a_duplicated_centre_stays_empty():
    from gpzoo_amd import ops
    X, C0 = K.tie_case()
    M = len(C0)
    got, _ = ops.kmeans_assign(cuda(X), cuda(C0, torch.float64))
    got = got.cpu().numpy()
    assert (got[:10] == 3).all() and (got[10:20] == 5).all()
    counts = np.bincount(got, minlength=M)
    assert counts[9] == 0 and counts[M - 1] == 0
    want_C, want_labels, _, moved = O.lloyd_iter(X, C0)
    C, labels, state = one_iteration(X, C0)
    np.testing.assert_array_equal(labels, want_labels)
    close(C, want_C)
    assert state[3] == len(moved) == 2


@pytest.mark.parametrize("n_empty", [1, 3])
def test_relocation_follows_the_oracles_pairing(n_empty):
    X, C0 = K.empty_case(n_empty)
    want_C, want_labels, _, moved = O.lloyd_iter(X, C0)
    C, labels, state = one_iteration(X, C0)
    np.testing.assert_array_equal(labels, want_labels)
    assert state[3] == n_empty == len(moved)
    for n, frm, to in moved:
        np.testing.assert_array_equal(C[to], X[n])                                     # the farthest point, exactly
    close(C, want_C)


def test_fewer_distinct_points_than_centres():
    from gpzoo.utilities import kmeans_inducing_points
    X, M = K.few_distinct_case()
    o = O.kmeans(X, M, random_state=0)
    C, info = kmeans_inducing_points(X, M, random_state=0, return_info=True)
    np.testing.assert_array_equal(info["seed_indices"], o["seed_indices"])             # the potential reaches 0: index 0
    assert info["inertia"] == 0.0 and np.isfinite(C).all() and info["n_iter"] == o["n_iter"]
    assert info["converged"] == o["converged"]
    np.testing.assert_array_equal(info["labels"], o["labels"])
    close(C, o["centres"])


@pytest.mark.parametrize("case", K.GOLDENS)
def test_seeding_picks_the_oracles_indices(case):
    from gpzoo_amd import ops
    z = golden(case)
    M = len(z["C0"])
    idx, C = ops.kmeans_seed(cuda(z["X"]), M, cuda(z["seed_u"]))
    np.testing.assert_array_equal(idx.cpu().numpy(), z["seed_idx"])
    np.testing.assert_array_equal(C.cpu().numpy(), z["X"].astype(np.float64)[z["seed_idx"]])
    if case == "40x40_d2_f64":
        assert sorted(idx.cpu().numpy().tolist()) == list(range(40))                   # M = N: every point once


def test_two_calls_agree_bit_for_bit():
    from gpzoo.utilities import kmeans_inducing_points
    z = golden("quality")
    a = kmeans_inducing_points(z["X"], 64, random_state=5, return_info=True)
    b = kmeans_inducing_points(z["X"], 64, random_state=5, return_info=True)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1]["labels"], b[1]["labels"])
    np.testing.assert_array_equal(a[1]["seed_indices"], b[1]["seed_indices"])
    assert a[1]["inertia"] == b[1]["inertia"] and a[1]["n_iter"] == b[1]["n_iter"]


def test_two_k_iterations_equal_k_plus_k():
    from gpzoo_amd import ops
    z = golden("5000x513_d2_f64")
    X = cuda(z["X"])

    def run(blocks):
        C = cuda(z["C0"], torch.float64).clone()
        labels = torch.full((len(z["X"]),), -1, dtype=torch.int32, device="cuda")
        state = ops.kmeans_state(X.device)
        for k in blocks:
            ops.kmeans_lloyd(X, C, labels, state, 0.0, k)
        return C.cpu().numpy(), labels.cpu().numpy(), state.cpu().numpy()

    a, b, c = run([6]), run([3, 3]), run([1] * 6)
    for other in (b, c):
        for x, y in zip(a, other):
            np.testing.assert_array_equal(x, y)
    assert a[2][0] == 6 and a[2][1] == 0


@pytest.mark.parametrize("block", [1, 10, 11, 16])
def test_block_boundaries_of_the_python_loop(block, monkeypatch):
    """The golden stops on its 11th iteration: inside a block of 16, on the last of a block of 11, on the first of the
    second block of 10 -- each the same as one iteration per call (the oracle's run, and bit for bit among themselves)."""
    import gpzoo_amd.utilities as U
    z = golden("1037x100_d2_f64")
    assert int(z["n_iter"]) == 11
    monkeypatch.setattr(U, "KMEANS_BLOCK", 1)
    want = U.kmeans_inducing_points(z["X"], 100, init=z["C0"], return_info=True)
    monkeypatch.setattr(U, "KMEANS_BLOCK", block)
    got = U.kmeans_inducing_points(z["X"], 100, init=z["C0"], return_info=True)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1]["labels"], want[1]["labels"])
    np.testing.assert_array_equal(got[1]["labels"], z["labels"])
    assert got[1]["n_iter"] == want[1]["n_iter"] == 11 and got[1]["converged"] == want[1]["converged"] == "labels"
    assert got[1]["inertia"] == want[1]["inertia"]


def test_stops_and_the_final_relabelling():
    """Labels: the returned labels are the last iteration's (w.r.t. the centres before its update); tol and max_iter: they are
    recomputed against the returned centres."""
    from gpzoo.utilities import kmeans_inducing_points
    for case, stop in (("1037x100_d2_f64", "labels"), ("1037x100_d2_f64_tol", "tol"), ("1037x100_d2_f64_it3", False)):
        z = golden(case)
        o = O.lloyd(z["X"], z["C0"], int(z["max_iter"]), float(z["tol"]))
        C, info = kmeans_inducing_points(z["X"], 100, init=z["C0"], max_iter=int(z["max_iter"]), tol=float(z["tol"]),
                                         return_info=True)
        assert info["converged"] == stop == o["converged"] and info["n_iter"] == o["n_iter"]
        assert o["relabelled"] == (stop != "labels")
        np.testing.assert_array_equal(info["labels"], o["labels"])
        if stop != "labels":
            np.testing.assert_array_equal(info["labels"], O.assign(z["X"], C)[0])
        assert info["inertia"] == pytest.approx(O.inertia_of(z["X"], C, info["labels"]), rel=1e-12)


def test_input_kinds_and_dtypes():
    from gpzoo.utilities import kmeans_inducing_points
    z = golden("1037x100_d2_f32")
    X, C0 = z["X"], z["C0"]
    a, ia = kmeans_inducing_points(X, 100, init=C0, return_info=True)
    b, ib = kmeans_inducing_points(torch.as_tensor(X), 100, init=torch.as_tensor(C0), return_info=True)
    c, ic = kmeans_inducing_points(torch.as_tensor(X).cuda(), 100, init=C0, return_info=True)
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and isinstance(ia["labels"], np.ndarray)
    assert isinstance(b, torch.Tensor) and not b.is_cuda and b.dtype == torch.float32 and not ib["labels"].is_cuda
    assert isinstance(c, torch.Tensor) and c.is_cuda and c.dtype == torch.float32 and ic["labels"].is_cuda
    assert ib["labels"].dtype == ic["labels"].dtype == torch.int64
    np.testing.assert_array_equal(a, b.numpy())
    np.testing.assert_array_equal(a, c.cpu().numpy())
    e = kmeans_inducing_points(X.astype(np.float64), 100, init=C0)
    assert e.dtype == np.float64 and e.shape == (100, 2)
    np.testing.assert_array_equal(e.astype(np.float32), a)                             # the float32 result is the rounded one
    for init in ("k-means++", "random"):
        f, info = kmeans_inducing_points(X, 100, init=init, random_state=3, return_info=True)
        assert f.shape == (100, 2) and info["seed_indices"].shape == (100,) and info["seed_indices"].dtype == np.int64
        assert len(np.unique(info["seed_indices"])) == 100
    np.testing.assert_array_equal(info["seed_indices"], np.random.default_rng(3).choice(len(X), 100, replace=False))
    with pytest.raises(ValueError, match="non-finite"):
        bad = torch.as_tensor(X).cuda().clone()
        bad[5, 1] = float("nan")
        kmeans_inducing_points(bad, 100)


def test_centres_serve_as_inducing_points_of_a_wsvgp():
    import torch.nn as nn
    from gpzoo.gp import WSVGP
    from gpzoo.kernels import RBF
    from gpzoo.utilities import kmeans_inducing_points
    z = golden("1037x100_d2_f32")
    X = torch.as_tensor(z["X"]).cuda()
    gp = WSVGP(RBF(), dim=2, M=100, jitter=1e-3).cuda()
    gp.Z = nn.Parameter(kmeans_inducing_points(X, 100, random_state=0))
    assert gp.Z.shape == (100, 2) and gp.Z.is_cuda and gp.Z.dtype == torch.float32
    qF = gp(X)[0]
    assert qF.mean.shape[-1] == len(X) and bool(torch.isfinite(qF.mean).all()) and bool(torch.isfinite(qF.scale).all())


def test_seeded_quality_matches_sklearns():
    """The mean final inertia over the fixture's 20 seeds lies within three of the fixture's standard errors of the mean of
    sklearn's own KMeans(init="k-means++", n_init=1) over 20 seeds."""
    from gpzoo.utilities import kmeans_inducing_points
    z = golden("quality")
    X = torch.as_tensor(z["X"]).cuda()
    got = np.array([kmeans_inducing_points(X, int(z["M"]), random_state=int(s), return_info=True)[1]["inertia"] for s in z["seeds"]])
    print("mean inertia", got.mean(), "sklearn", float(z["sklearn_mean"]), "oracle", float(z["oracle_mean"]), "se", float(z["se_diff"]))
    assert abs(got.mean() - float(z["sklearn_mean"])) <= 3 * float(z["se_diff"])


def test_ops_reject_bad_arguments():
    from gpzoo_amd import ops
    X, C = torch.zeros(10, 2).cuda(), torch.zeros(3, 2, dtype=torch.float64).cuda()
    labels, state = torch.zeros(10, dtype=torch.int32).cuda(), ops.kmeans_state(X.device)
    with pytest.raises(ValueError, match="kmeans_lloyd"):
        ops.kmeans_lloyd(X, C.float(), labels, state, 0.0, 1)
    with pytest.raises(ValueError, match="kmeans_lloyd"):
        ops.kmeans_lloyd(X, C, labels.long(), state, 0.0, 1)
    with pytest.raises(RuntimeError, match="iters=0"):
        ops.kmeans_lloyd(X, C, labels, state, 0.0, 0)
    with pytest.raises(ValueError, match="gpz_kmeans_assign"):
        ops.kmeans_assign(torch.zeros(10, 5).cuda(), torch.zeros(3, 5, dtype=torch.float64).cuda())
    with pytest.raises(ValueError, match="kmeans_seed"):
        ops.kmeans_seed(X, 3, torch.zeros(4, 2, dtype=torch.float64).cuda())
    with pytest.raises(ValueError, match="gpz_kmeans_seed"):
        ops.kmeans_seed(X, 11, torch.zeros(11, 2, dtype=torch.float64).cuda())
