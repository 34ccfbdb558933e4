"""CPU: project_factors_to_inducing -- the argument checks that come before any GPU use, the public surface, the C ABI's
host-side refusals and plan / workspace queries, and the torch oracle (tests/projection_oracle.py) against the fixtures the
notebook's composition produced on the reference's kernels (no launch: there is no GPU here)."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import projection_cases as PC
import projection_oracle as PO
from conftest import GOLDEN, ROOT

SYMBOLS = ("gpz_kernel_gram", "gpz_kernel_gram_workspace_bytes", "gpz_kernel_gram_plan")


def golden(name):
    return np.load(os.path.join(GOLDEN, f"extra_projection_{name}.npz"))


def _kernels():
    from gpzoo import kernels as K
    return K


def _bad_calls():
    K = _kernels()
    rng = np.random.default_rng(0)
    Z, X, F = rng.random((7, 2)), rng.random((50, 2)), rng.random((3, 50))
    nan, inf = X.copy(), F.copy().astype(np.float32)
    nan[7, 1], inf[1, 3] = np.nan, np.inf
    k = K.RBF(1.0, 0.5)
    knan = K.RBF(float("nan"), 0.5)
    return [
        ((k, Z[0], X, F), {}, "Z must be"), ((k, Z, X[:, 0], F), {}, "X must be"), ((k, Z, X, F[0]), {}, "F must be"),
        ((k, Z, X, F[None]), {}, "F must be"),
        ((k, rng.random((7, 3)), X, F), {}, "coordinates per point"),
        ((k, rng.random((7, 5)), rng.random((50, 5)), F), {}, "dimension 5"),
        ((k, rng.random((7, 0)), rng.random((50, 0)), F), {}, "dimension 0"),
        ((k, Z, X[:49], F), {}, "columns of F"), ((k, Z, X, F[:, :49]), {}, "columns of F"),
        ((k, Z, X[:0], F[:, :0]), {}, "N=0"), ((k, Z[:0], X, F), {}, "M=0"), ((k, Z, X, F[:0]), {}, "L=0"),
        ((k, rng.random((8193, 2)), X, F), {}, "M=8193"),
        ((K.NSF_RBF(L=4), Z, X, F), {}, "4 latents, F has 3 rows"),
        ((K.batched_Matern32(sigma=[1.0, 2.0], lengthscale=[1.0, 2.0]), Z, X, F), {}, "2 latents, F has 3 rows"),
        ((k, Z, X, F), dict(jitter=-1e-5), "jitter"), ((k, Z, X, F), dict(jitter=float("nan")), "jitter"),
        ((k, Z, X, F), dict(kzz_jitter=-1.0), "kzz_jitter"), ((k, Z, X, F), dict(jitter="1e-5"), "jitter"),
        ((k, Z, nan, F), {}, "non-finite"), ((k, Z, X, inf), {}, "non-finite"), ((knan, Z, X, F), {}, "non-finite"),
    ]


@pytest.mark.parametrize("args,kw,word", _bad_calls())
@pytest.mark.parametrize("kind", ["numpy", "tensor"])
def test_bad_arguments_raise_before_any_gpu_use(args, kw, word, kind, monkeypatch):
    from gpzoo.utilities import project_factors_to_inducing
    from gpzoo_amd import _lib

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the arguments were checked")

    monkeypatch.setattr(torch.cuda, "current_device", no_gpu)
    monkeypatch.setattr(torch.Tensor, "to", no_gpu)
    monkeypatch.setattr(_lib, "load", no_gpu)
    if kind == "tensor":
        args = (args[0],) + tuple(torch.as_tensor(a) for a in args[1:])
    with pytest.raises(ValueError, match=word):
        project_factors_to_inducing(*args, **kw)


def test_unsupported_kernels_are_refused_before_any_gpu_use(monkeypatch):
    from gpzoo.utilities import project_factors_to_inducing
    from gpzoo_amd import _lib
    K = _kernels()

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the kernel was checked")

    monkeypatch.setattr(torch.cuda, "current_device", no_gpu)
    monkeypatch.setattr(_lib, "load", no_gpu)
    rng = np.random.default_rng(0)
    Z, X, F = rng.random((7, 2)), rng.random((50, 2)), rng.random((3, 50))
    for mg in (K.MGGP_RBF(), K.MGGP_NSF_RBF(L=3), K.batched_MGGP_RBF()):
        with pytest.raises(NotImplementedError, match="multi-group"):
            project_factors_to_inducing(mg, Z, X, F)

    class Mine(K.batched_RBF):
        def covariance(self, x1, x2):
            return (x1 * x2).sum()

    with pytest.raises(NotImplementedError, match="user-defined"):
        project_factors_to_inducing(Mine(), Z, X, F)
    with pytest.raises(TypeError, match="not a kernel"):
        project_factors_to_inducing(torch.nn.Linear(2, 2), Z, X, F)


def test_name_resolves_with_the_documented_signature():
    import gpzoo.utilities as G
    import gpzoo_amd.utilities as U
    assert G.project_factors_to_inducing is U.project_factors_to_inducing
    assert "project_factors_to_inducing" not in U._NOT_REBUILT
    E = inspect.Parameter.empty
    ps = inspect.signature(U.project_factors_to_inducing).parameters
    assert [(n, p.default) for n, p in ps.items()] == [("kernel", E), ("Z", E), ("X", E), ("F", E), ("jitter", 1e-5),
                                                       ("whitened", False), ("kzz_jitter", 0.0), ("return_info", False)]
    assert all(p.kind == inspect.Parameter.KEYWORD_ONLY for n, p in ps.items() if n not in ("kernel", "Z", "X", "F"))
    doc = U.project_factors_to_inducing.__doc__
    for word in ("loses its digits", "gp.jitter", "bit for bit", "LinAlgError", "residual"):
        assert word in doc, word


def test_symbols_are_bound_and_declared():
    from gpzoo_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "gpzoo_hip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.exported_symbols()
        assert f"{name}(" in hdr
    assert "#define GPZ_VERSION 212" in hdr
    assert "gram.hip" in build.SOURCES


def test_ops_need_cuda_tensors():
    from gpzoo_amd import _lib, ops
    spec = ops.KernelSpec(_lib.KERNEL_RBF, torch.ones(1), torch.ones(1), False)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.kernel_gram(spec, torch.zeros(3, 2), torch.zeros(5, 2), torch.zeros(2, 5))


def _lib_built():
    from gpzoo_amd import _lib, build
    build.build(force=False, verbose=False)
    return _lib.load()


def test_entry_rejects_bad_arguments_on_the_host():
    """Host checks only (no launch: every call fails them; the buffers are never dereferenced)."""
    from gpzoo_amd._lib import KernelDesc
    lib = _lib_built()
    buf = ctypes.c_void_p(16)
    ok = dict(kind=0, n_latent=2, dtype=0, Z=buf, M=40, X=buf, N=300, d=2, F=buf, R=1, jitter=1e-5, G=buf, b=buf, ws=buf,
              ws_bytes=1 << 40)

    def gram(**kw):
        a = dict(ok, **kw)
        desc = KernelDesc()
        desc.kind, desc.n_latent, desc.dtype, desc.sigma, desc.lengthscale = a["kind"], a["n_latent"], a["dtype"], 16, 16
        return lib.gpz_kernel_gram(ctypes.byref(desc), a["Z"], a["M"], a["X"], a["N"], a["d"], a["F"], a["R"], a["jitter"], a["G"],
                                   a["b"], a["ws"], a["ws_bytes"], None)

    bad = [(dict(kind=2), b"kind 2"), (dict(kind=3), b"kind 3"), (dict(kind=6), b"kind 6"), (dict(d=5), b"dimension 5"),
           (dict(d=0), b"dimension 0"), (dict(R=65), b"R=65"), (dict(R=0), b"R=0"), (dict(N=0), b"N=0"), (dict(N=1 << 31), b"N="),
           (dict(M=0), b"M=0"), (dict(M=8193), b"M=8193"), (dict(n_latent=0), b"n_latent=0"), (dict(dtype=2), b"dtype"),
           (dict(jitter=-1.0), b"jitter"), (dict(jitter=float("nan")), b"jitter"), (dict(Z=None), b"null"),
           (dict(F=None), b"null"), (dict(G=None), b"null"), (dict(ws=None), b"workspace"), (dict(ws_bytes=64), b"workspace")]
    for kw, msg in bad:
        assert gram(**kw) < 0, kw
        err = lib.gpz_last_error()
        assert msg in err and b"gpz_kernel_gram" in err, (kw, err)
    assert lib.gpz_kernel_gram(None, buf, 40, buf, 300, 2, buf, 1, 0.0, buf, buf, buf, 1 << 40, None) < 0
    for args in ((0, 40, 2, 1, 0), (300, 0, 2, 1, 0), (300, 8193, 2, 1, 0), (300, 40, 2, 65, 0), (300, 40, 2, 1, 2)):
        assert lib.gpz_kernel_gram_workspace_bytes(*args) == 0, args


def test_plan_splits_cover_n_exactly_and_bound_a_split():
    from gpzoo_amd import ops
    for dt, step in ((torch.float32, 32), (torch.float64, 16)):
        for N, M, n in ((1, 1, 1), (300, 40, 1), (1037, 529, 4), (39694, 3000, 10), (200000, 2048, 32), (200000, 1, 1),
                        (2 ** 31 - 1, 128, 1)):
            p = ops.kernel_gram_plan(N, M, n, dt)
            assert p["tile"] == 128 and p["col_step"] == step
            assert p["cols_per_split"] % step == 0 and p["cols_per_split"] >= 4 * step
            assert (p["n_splits"] - 1) * p["cols_per_split"] < N <= p["n_splits"] * p["cols_per_split"]
            assert p["cols_per_split"] <= 16384 + step        # an fp32 partial sum has at most this many terms
    with pytest.raises(ValueError, match="M=8193"):
        ops.kernel_gram_plan(100, 8193, 1, torch.float32)


def test_workspace_holds_partial_tiles_only():
    """The blocking condition of the feature: at the notebook's shape the workspace is smaller than the split count times
    G itself, and for a fixed number of splits it does not depend on N."""
    from gpzoo_amd import ops
    N, M, L = 39694, 3000, 10
    for dt, esz in ((torch.float32, 4), (torch.float64, 8)):
        p = ops.kernel_gram_plan(N, M, L, dt)
        ws = p["workspace_bytes"](1)
        assert 0 < ws < p["n_splits"] * L * M * M * 8
        nt = -(-M // p["tile"])
        want = p["n_splits"] * L * (nt * (nt + 1) // 2 * p["tile"] ** 2 + nt * 16 * p["tile"]) * esz
        assert want <= ws <= want + 1024                                  # the stated bound, plus alignment
        assert ws < N * M * L * esz / 4                                    # a fraction of a stored K_zx
        same = [q for q in (ops.kernel_gram_plan(n, M, L, dt) for n in range(N - 3000, N + 3000, 500)) if q["n_splits"] == p["n_splits"]]
        assert len(same) >= 6 and {q["workspace_bytes"](1) for q in same} == {ws}
    p3 = ops.kernel_gram_plan(200000, 2048, 32, torch.float32)
    assert p3["workspace_bytes"](1) < p3["n_splits"] * 32 * 2048 * 2048 * 8


@pytest.mark.parametrize("name", sorted(PC.GOLDENS))
def test_oracle_reproduces_the_reference_composition(name):
    z = golden(name)
    N, M, L, frac, cls, per_latent = PC.GOLDENS[name]
    o = PO.project(PC.GOLDEN_KIND[cls], z["Z"], z["X"], z["F"], torch.as_tensor(z["sigma"]), torch.as_tensor(z["lengthscale"]),
                   jitter=float(z["jitter"]))
    b = o["b"][:, 0] if per_latent else o["b"][0]
    for got, key in ((o["mu"], "mu"), (o["alpha"], "alpha"), (b, "b")):
        ref = z[key]
        assert np.abs(got.numpy() - ref).max() <= 1e-10 * np.abs(ref).max(), key
    # the residual the function reports (from G, b and alpha alone) is the definition's, to the digits the difference keeps
    G0 = o["G"] - float(z["jitter"]) * torch.eye(M, dtype=torch.float64)
    a, F = o["alpha"], torch.as_tensor(z["F"]).double()
    Ga = (G0 @ a[:, :, None])[:, :, 0] if per_latent else a @ G0[0]
    short = ((F * F).sum(1) - 2 * (a * b).sum(1) + (a * Ga).sum(1)) / (F * F).sum(1)
    assert (short - o["residual"]).abs().max() < 1e-9
    assert 0 < float(o["residual"].min()) and float(o["residual"].max()) < 0.9
