"""CPU: the numpy oracle of kmeans_inducing_points against every sklearn golden, the conditions the goldens were written
under, the seeding quality fixture, the argument checks that come before any GPU use, the public surface, and the host-side
refusals of the three C entries (no launch: there is no GPU here)."""
import inspect
import os

import numpy as np
import pytest
import torch

import kmeans_cases as K
import kmeans_oracle as O
from conftest import GOLDEN, ROOT

SYMBOLS = ("gpz_kmeans_seed", "gpz_kmeans_seed_workspace_bytes", "gpz_kmeans_lloyd", "gpz_kmeans_lloyd_workspace_bytes",
           "gpz_kmeans_assign", "gpz_kmeans_assign_workspace_bytes")


def golden(name):
    return np.load(os.path.join(GOLDEN, f"extra_kmeans_{name}.npz"))


@pytest.fixture(scope="module")
def runs():
    """The oracle's run of every golden, once."""
    out = {}
    for case in K.GOLDENS:
        z = golden(case)
        out[case] = O.lloyd(z["X"], z["C0"], int(z["max_iter"]), float(z["tol"]), gap=True)
    return out


@pytest.mark.parametrize("case", K.GOLDENS)
def test_oracle_reproduces_sklearn(case, runs):
    """Labels and n_iter exact; centres and inertia to 1e-12 for float64 data; for float32 data to 1e-12 against sklearn's
    run on the float64 cast of the same values and to 1e-5 against its float32 run."""
    z, o = golden(case), runs[case]
    np.testing.assert_array_equal(o["labels"], z["labels"])
    assert o["n_iter"] == int(z["n_iter"])
    scale = np.abs(z["centers"]).max()
    if case.endswith("f32"):
        np.testing.assert_array_equal(o["labels"], z["labels64"])                      # condition (c)
        assert o["n_iter"] == int(z["n_iter64"])
        np.testing.assert_allclose(o["centres"], z["centers64"], rtol=0, atol=1e-12 * scale)
        assert o["inertia"] == pytest.approx(float(z["inertia64"]), rel=1e-12)
        np.testing.assert_allclose(o["centres"], z["centers"], rtol=0, atol=1e-5 * scale)
        assert o["inertia"] == pytest.approx(float(z["inertia"]), rel=1e-5)
    else:
        np.testing.assert_allclose(o["centres"], z["centers"], rtol=0, atol=1e-12 * scale)
        assert o["inertia"] == pytest.approx(float(z["inertia"]), rel=1e-12, abs=1e-12 * scale ** 2)


def test_goldens_hold_what_the_gpu_tests_rely_on(runs):
    """Conditions (a)-(c) of the generator, the coverage the list claims, and the seeding fixtures' margins."""
    seen_d, seen_t = set(), set()
    for case in K.GOLDENS:
        z, o = golden(case), runs[case]
        assert o["min_gap"] > 1e-9, case                                               # condition (b)
        N, d = z["X"].shape
        M = len(z["C0"])
        seen_d.add(d)
        seen_t.add(z["X"].dtype)
        assert z["C0"].dtype == np.float64 and z["centers"].dtype == z["X"].dtype and z["labels"].shape == (N,)
        assert (case.endswith("f32")) == (z["X"].dtype == np.float32) == ("labels64" in z.files)
        if case in K.GOLDEN_STOP:
            assert o["converged"] == K.GOLDEN_STOP[case], case
        u = z["seed_u"]
        assert u.shape == (M, O.n_trials(M)) and (0 <= u).all() and (u < 1).all()
        idx, draw_margin, win_margin = O.seed(z["X"], M, u)
        np.testing.assert_array_equal(idx, z["seed_idx"])
        assert draw_margin > 1e-9 and win_margin > 1e-9, case
    assert seen_d == {1, 2, 3, 4} and seen_t == {np.dtype(np.float32), np.dtype(np.float64)}
    stops = {runs[c]["converged"] for c in K.GOLDENS}
    assert stops == {"labels", "tol", False}
    assert runs["1037x100_d2_f64_tol"]["n_iter"] > 1 and runs["1037x100_d2_f64_it3"]["n_iter"] == 3
    z = golden("40x40_d2_f64")
    assert len(z["X"]) == len(z["C0"]) == 40 and len(np.unique(z["X"], axis=0)) == 40
    assert sorted(z["seed_idx"].tolist()) == list(range(40))                           # M = N: every point once
    assert len(golden("500x1_d2_f64")["C0"]) == 1
    assert len(golden("5000x513_d2_f64")["C0"]) == 2 * K.T_C + 1
    z = golden("600x20_d2_f64_empty")                                                  # one empty cluster, first iteration
    _, labels, _, moved = O.lloyd_iter(z["X"], z["C0"])
    assert len(moved) == 1 and moved[0][2] == 3 and runs["600x20_d2_f64_empty"]["relocated"] == 1


def test_seeding_quality_of_the_oracle_matches_sklearn():
    """The final inertia of seed + Lloyd over 20 seeds against sklearn's own k-means++ over 20 seeds: the means agree
    within three standard errors of their difference (the draws differ, the algorithm and its quality do not)."""
    z = golden("quality")
    assert len(z["seeds"]) == 20 and z["X"].shape == (2000, 2) and int(z["M"]) == 64
    a, b = z["sklearn_inertia"], z["oracle_inertia"]
    assert float(z["sklearn_mean"]) == pytest.approx(a.mean()) and float(z["oracle_mean"]) == pytest.approx(b.mean())
    assert float(z["se_diff"]) == pytest.approx(np.sqrt(a.var(ddof=1) / 20 + b.var(ddof=1) / 20))
    assert abs(b.mean() - a.mean()) <= 3 * float(z["se_diff"])
    o = O.kmeans(z["X"], 64, random_state=int(z["seeds"][3]))                          # the fixture is the oracle's
    assert o["inertia"] == pytest.approx(b[3], rel=1e-12)


def _bad_calls():
    rng = np.random.default_rng(0)
    X = rng.random((50, 2))
    nan, inf = X.copy(), X.copy().astype(np.float32)
    nan[7, 1], inf[3, 0] = np.nan, np.inf
    return [
        ((X[:, 0], 5), {}, "X must be"), ((X[None], 5), {}, "X must be"),
        ((rng.random((50, 0)), 5), {}, "dimension 0"), ((rng.random((50, 5)), 5), {}, "dimension 5"),
        ((X, 0), {}, "M=0"), ((X, 51), {}, "M=51"), ((X, 2.5), {}, "M must be"),
        ((nan, 5), {}, "non-finite"), ((inf, 5), {}, "non-finite"),
        ((X, 5), dict(init=rng.random((4, 2))), "init must be"), ((X, 5), dict(init=rng.random((5, 3))), "init must be"),
        ((X, 5), dict(init=np.full((5, 2), np.nan)), "init holds"),
        ((X, 5), dict(init="kmeans++"), "unknown init"),
        ((X, 5), dict(max_iter=0), "max_iter"), ((X, 5), dict(max_iter=2.5), "max_iter"),
        ((X, 5), dict(tol=-1e-4), "tol"), ((X, 5), dict(tol=float("nan")), "tol"),
    ]


@pytest.mark.parametrize("args,kw,word", _bad_calls())
@pytest.mark.parametrize("kind", ["numpy", "tensor"])
def test_bad_arguments_raise_before_any_gpu_use(args, kw, word, kind, monkeypatch):
    from gpzoo.utilities import kmeans_inducing_points
    from gpzoo_amd import _lib

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the arguments were checked")

    monkeypatch.setattr(torch.cuda, "current_device", no_gpu)
    monkeypatch.setattr(torch.Tensor, "to", no_gpu)
    monkeypatch.setattr(_lib, "load", no_gpu)
    if kind == "tensor":
        args = (torch.as_tensor(args[0]),) + args[1:]
        kw = {k: torch.as_tensor(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    with pytest.raises(ValueError, match=word):
        kmeans_inducing_points(*args, **kw)


def test_name_resolves_with_the_documented_signature():
    import gpzoo.utilities as G
    import gpzoo_amd.utilities as U
    assert G.kmeans_inducing_points is U.kmeans_inducing_points and "kmeans_inducing_points" not in U._NOT_REBUILT
    E = inspect.Parameter.empty
    ps = inspect.signature(U.kmeans_inducing_points).parameters
    assert [(n, p.default) for n, p in ps.items()] == [("X", E), ("M", E), ("init", "k-means++"), ("max_iter", 300), ("tol", 1e-4),
                                                       ("random_state", None), ("return_info", False)]
    assert all(p.kind == inspect.Parameter.KEYWORD_ONLY for n, p in ps.items() if n not in ("X", "M"))
    doc = U.kmeans_inducing_points.__doc__
    for word in ('n_init=1', 'algorithm="lloyd"', "DIFFERS from sklearn", "d <= 4", "2**31", "dense", "sample weights"):
        assert word in doc, word


def test_the_package_imports_no_sklearn():
    """In a fresh interpreter (this process has imported sklearn for other tests): importing the package and running the
    argument checks of kmeans_inducing_points pulls in no sklearn."""
    import subprocess
    import sys
    code = ("import sys, numpy as np\n"
            "import gpzoo_amd.ops\n"
            "from gpzoo.utilities import kmeans_inducing_points\n"
            "try:\n    kmeans_inducing_points(np.zeros((4, 2)), 5)\nexcept ValueError:\n    pass\n"
            "assert not any(m == 'sklearn' or m.startswith('sklearn.') for m in sys.modules)\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT, timeout=300)


def test_symbols_are_bound_and_declared():
    from gpzoo_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "gpzoo_hip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.exported_symbols()
        assert f"{name}(" in hdr
    assert "#define GPZ_VERSION 212" in hdr and "gpz_kmeans_state" in hdr
    assert "kmeans.hip" in build.SOURCES and "-ffp-contract=off" in build.SOURCE_FLAGS["kmeans.hip"]


def test_ops_need_cuda_tensors():
    from gpzoo_amd import ops
    X, C = torch.zeros(5, 2), torch.zeros(2, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.kmeans_seed(X, 2, torch.zeros(2, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.kmeans_lloyd(X, C, torch.zeros(5, dtype=torch.int32), torch.zeros(4, dtype=torch.int64), 0.0, 1)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.kmeans_assign(X, C)


def _lib_built():
    from gpzoo_amd import _lib, build
    build.build(force=False, verbose=False)
    return _lib.load()


def test_entries_reject_bad_arguments_on_the_host():
    """Host checks only (no launch: every call fails them; the buffers are never dereferenced)."""
    import ctypes
    lib = _lib_built()
    buf = ctypes.c_void_p(16)
    big = 1 << 40
    ok = dict(X=buf, N=100, d=2, dtype=0, M=7, T=3, u=buf, idx=buf, C=buf, tol=0.0, iters=4, labels=buf, state=buf, keep=0,
              d2=None, inertia=None, ws=buf, ws_bytes=big, stream=None)

    def seed(**kw):
        a = dict(ok, **kw)
        return lib.gpz_kmeans_seed(a["X"], a["N"], a["d"], a["dtype"], a["M"], a["T"], a["u"], a["idx"], a["C"], a["ws"],
                                   a["ws_bytes"], a["stream"])

    def lloyd(**kw):
        a = dict(ok, **kw)
        return lib.gpz_kmeans_lloyd(a["X"], a["N"], a["d"], a["dtype"], a["C"], a["M"], a["tol"], a["iters"], a["labels"],
                                    a["state"], a["ws"], a["ws_bytes"], a["stream"])

    def assign(**kw):
        a = dict(ok, **kw)
        return lib.gpz_kmeans_assign(a["X"], a["N"], a["d"], a["dtype"], a["C"], a["M"], a["keep"], a["labels"], a["d2"],
                                     a["inertia"], a["ws"], a["ws_bytes"], a["stream"])

    shared = [(dict(X=None), b"null"), (dict(C=None), b"null"), (dict(ws=None), b"null"), (dict(d=0), b"d=0"), (dict(d=5), b"d=5"),
              (dict(dtype=2), b"dtype"), (dict(N=0, M=0), b"N=0"), (dict(N=1 << 31), b"N="), (dict(M=0), b"M=0"),
              (dict(M=101), b"M=101"), (dict(ws_bytes=16), b"workspace")]
    table = [(seed, b"gpz_kmeans_seed", shared + [(dict(u=None), b"null"), (dict(idx=None), b"null"), (dict(T=0), b"T=0"),
                                                  (dict(T=33), b"T=33")]),
             (lloyd, b"gpz_kmeans_lloyd", shared + [(dict(labels=None), b"null"), (dict(state=None), b"null"),
                                                    (dict(tol=-1.0), b"tol_abs"), (dict(tol=float("nan")), b"tol_abs"),
                                                    (dict(iters=0), b"iters=0")]),
             (assign, b"gpz_kmeans_assign", shared + [(dict(labels=None), b"null"), (dict(keep=2), b"keep_labels=2")])]
    for call, who, bad in table:
        for kw, msg in bad:
            assert call(**kw) < 0, (who, kw)
            err = lib.gpz_last_error()
            assert msg in err and who in err, (who, kw, err)
    assert lib.gpz_kmeans_lloyd_workspace_bytes(100, 2, 7) >= 100 * 2 * 8
    assert lib.gpz_kmeans_assign_workspace_bytes(100, 2, 7) >= 100 * 2 * 8
    assert lib.gpz_kmeans_seed_workspace_bytes(100, 2, 7, 3) >= 100 * 3 * 8
    # the centre split of a small N asks for its (d^2, index) pairs: 12 bytes per point and split
    p = K.split_plan(K.B_N + 1, 2 * K.T_C + 1)
    one = lib.gpz_kmeans_assign_workspace_bytes(2 * K.T_C + 1, 2, K.T_C)
    assert p["splits"] == 3 and lib.gpz_kmeans_assign_workspace_bytes(2 * K.T_C + 1, 2, 2 * K.T_C + 1) > one
    for name, args in (("gpz_kmeans_lloyd_workspace_bytes", (100, 5, 7)), ("gpz_kmeans_lloyd_workspace_bytes", (100, 2, 0)),
                       ("gpz_kmeans_lloyd_workspace_bytes", (100, 2, 101)), ("gpz_kmeans_lloyd_workspace_bytes", (0, 2, 1)),
                       ("gpz_kmeans_assign_workspace_bytes", (100, 0, 7)), ("gpz_kmeans_assign_workspace_bytes", (1 << 31, 2, 7)),
                       ("gpz_kmeans_seed_workspace_bytes", (100, 2, 7, 0)), ("gpz_kmeans_seed_workspace_bytes", (100, 2, 7, 33)),
                       ("gpz_kmeans_seed_workspace_bytes", (100, 2, 101, 3))):
        assert getattr(lib, name)(*args) == 0, (name, args)
        assert name.encode() in lib.gpz_last_error()
