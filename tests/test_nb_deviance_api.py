"""CPU: the surface of the NB deviance -- the C ABI's new symbols and host-only queries, the argument checks that return
before any launch (through ctypes, with pointers that are never dereferenced), the Python names, and the validation of
``deviance(family=..., theta=...)`` on CPU tensors."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpz_nb_deviance", "gpz_nb_deviance_workspace_bytes", "gpz_nb_deviance_plan",
       "gpz_nb_deviance_sparse", "gpz_nb_deviance_sparse_workspace_bytes", "gpz_nb_deviance_sparse_plan")
MODELS = ("NSF", "NSF2", "MGGP_NSF", "Hybrid_NSF2", "Hybrid_NSF_Exact", "Hybrid_NSF")


def test_new_symbols_are_bound_and_declared_under_version_212():
    from gpzoo_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "gpzoo_hip.h")).read()
    assert re.search(r"^#define GPZ_VERSION 212$", header, re.M)
    for name in NEW:
        assert name in _lib.exported_symbols(), name
        assert re.search(r"\b%s\(" % name, header), name
    assert "nb_deviance.hip" in build.SOURCES


def test_plan_queries_answer_without_a_device():
    from gpzoo_amd import ops
    N, D, Lt = 7000, 17702, 20
    p = ops.nb_deviance_plan(N, D, Lt)
    assert p["spots_per_tile"] > 0 and p["genes_per_tile"] > 0 and p["genes_per_block"] % p["genes_per_tile"] == 0
    assert p["gene_slices"] == -(-D // p["genes_per_block"]) and p["factors_padded"] >= Lt
    assert p["spot_slices"] * p["tiles_per_spot_slice"] >= -(-N // p["spots_per_tile"])
    nnz = D * N // 20
    s = ops.nb_deviance_sparse_plan(39694, N, D, Lt, nnz)
    assert s["gene_chunk"] > 0 and s["n_gene_chunks"] >= D and s["factors_padded"] >= Lt
    # nothing of D x B elements in either workspace
    assert 0 < p["workspace_bytes"] < 4 * D * N and 0 < s["workspace_bytes"] < 4 * D * N
    # nor of nnz elements in the sparse one: it grows by the chunk list alone
    more = ops.nb_deviance_sparse_plan(39694, N, D, Lt, 2 * nnz)["workspace_bytes"]
    assert more - s["workspace_bytes"] < nnz // 4
    for bad in (0, 65):
        with pytest.raises(ValueError, match="factors"):
            ops.nb_deviance_plan(100, 50, bad)
        with pytest.raises(ValueError, match="factors"):
            ops.nb_deviance_sparse_plan(100, 100, 50, bad, 10)


def _fake(n=1):
    """Aligned non-null addresses for arguments the entries check and never dereference on the host."""
    return [C.c_void_p(0x10000 * (i + 1)) for i in range(n)]


def test_dense_argument_errors_return_before_any_launch():
    from gpzoo_amd import _lib
    lib = _lib.load()
    N, D, Lt = 130, 80, 5
    need = lib.gpz_nb_deviance_workspace_bytes(N, D, Lt)
    assert need > 0

    def call(ptrs=None, Lt=Lt, N=N, ws=C.c_void_p(0x900000), ws_bytes=need):
        p = _fake(13) if ptrs is None else ptrs
        return lib.gpz_nb_deviance(*p[:6], N, D, Lt, 1, *p[6:13], ws, ws_bytes, None)

    def refused(rc, word):
        assert rc == -1
        assert word in lib.gpz_last_error().decode()

    refused(call(Lt=0), "factors")
    refused(call(Lt=65), "factors")
    refused(call(N=0), "extents")
    assert lib.gpz_nb_deviance_workspace_bytes(N, D, 0) == 0 and lib.gpz_nb_deviance_workspace_bytes(N, D, 65) == 0
    assert lib.gpz_nb_deviance_workspace_bytes(0, D, Lt) == 0
    for k in range(13):
        p = _fake(13)
        p[k] = None
        refused(call(ptrs=p), "theta is missing" if k == 4 else "null pointer")
    refused(call(ws=None), "null pointer")
    refused(call(ws_bytes=need - 1), "workspace")
    p = _fake(13)
    p[2] = C.c_void_p(0x30004)                       # W
    refused(call(ptrs=p), "aligned")
    refused(call(ws=C.c_void_p(0x900008)), "aligned")


def test_sparse_argument_errors_return_before_any_launch():
    from gpzoo_amd import _lib
    lib = _lib.load()
    N, B, D, Lt, nnz = 130, 37, 80, 5, 900
    need = lib.gpz_nb_deviance_sparse_workspace_bytes(N, B, D, nnz, Lt)
    assert need > 0

    def call(ptrs=None, B=B, Lt=Lt, ws=C.c_void_p(0x900000), ws_bytes=need, nnz=nnz):
        p = _fake(20) if ptrs is None else ptrs
        return lib.gpz_nb_deviance_sparse(*p[:13], N, B, D, nnz, Lt, 1, *p[13:20], ws, ws_bytes, None)

    def refused(rc, word):
        assert rc == -1
        assert word in lib.gpz_last_error().decode()

    refused(call(Lt=0), "factors")
    refused(call(Lt=65), "factors")
    refused(call(B=N + 1), "distinct spots")
    assert lib.gpz_nb_deviance_sparse_workspace_bytes(N, B, D, nnz, 65) == 0
    assert lib.gpz_nb_deviance_sparse_workspace_bytes(N, N + 1, D, nnz, Lt) == 0
    for k in (0, 1, 2, 3, 4, 5, 8, 13, 14, 15, 16, 17, 18, 19):
        p = _fake(20)
        p[k] = None
        refused(call(ptrs=p), "theta is missing" if k == 4 else "null pointer")
    p = _fake(20)
    p[6] = None                                      # col_gene with nnz > 0
    refused(call(ptrs=p), "null pointer")
    p = _fake(20)
    p[11] = None                                     # idx without pos
    refused(call(ptrs=p), "idx and pos")
    p = _fake(20)
    p[11] = p[12] = None                             # no view, but B < N
    refused(call(ptrs=p), "needs idx and pos")
    refused(call(ws=None), "null pointer")
    refused(call(ws_bytes=need - 1), "workspace")
    p = _fake(20)
    p[2] = C.c_void_p(0x30004)
    refused(call(ptrs=p), "aligned")
    refused(call(ws=C.c_void_p(0x900008)), "aligned")


def test_python_names_resolve_through_the_shims():
    import gpzoo.likelihoods as L
    import gpzoo_amd.likelihoods as AL
    from gpzoo_amd import ops
    assert L.nb_deviance is AL.nb_deviance and L.NBDeviance is AL.NBDeviance
    assert AL.NBDeviance._fields[:10] == AL.PoissonDeviance._fields
    assert AL.NBDeviance._fields[10:] == ("loglik", "loglik_per_gene", "loglik_per_spot", "poisson_loglik",
                                          "poisson_loglik_per_gene", "theta")
    assert list(inspect.signature(AL.nb_deviance).parameters) == ["qF_list", "W_list", "V_pos", "theta_pos", "y", "lognormal_mean"]
    assert inspect.signature(AL.nb_deviance).parameters["lognormal_mean"].kind is inspect.Parameter.KEYWORD_ONLY
    for name in ("nb_deviance", "nb_deviance_sparse", "nb_deviance_plan", "nb_deviance_sparse_plan"):
        assert callable(getattr(ops, name)), name
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.nb_deviance(torch.zeros(2, 3), torch.ones(2, 3), torch.ones(4, 2), torch.ones(3), torch.ones(4), torch.ones(4, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.nb_deviance_sparse(torch.zeros(2, 3), torch.ones(2, 3), torch.ones(4, 2), torch.ones(3), torch.ones(4),
                               AL.SparseCounts(torch.ones(4, 3)))


@pytest.mark.parametrize("cls", MODELS)
def test_deviance_signatures_end_with_family_and_theta(cls):
    import gpzoo.likelihoods as L
    params = list(inspect.signature(getattr(L, cls).deviance).parameters.values())
    named = [p for p in params if p.kind is not inspect.Parameter.VAR_KEYWORD]
    assert [p.name for p in named[-2:]] == ["family", "theta"]
    assert named[-2].default == "poisson" and named[-1].default is None
    # what was there before keeps its place
    lead = ["self", "X", "y"] + (["groupsX"] if cls == "MGGP_NSF" else []) + ["idx", "V", "lognormal_mean"]
    assert [p.name for p in named[:-2]] == lead


def _cpu_models():
    import gpzoo.gp as G
    import gpzoo.kernels as K
    from gpzoo.likelihoods import NSF, NSF2, Hybrid_NSF, Hybrid_NSF2
    y = torch.ones(6, 9)
    def gp():
        g = G.WSVGP(K.NSF_RBF(L=2, lengthscale=2.0), dim=2, M=4, jitter=1e-2)
        g.mu = torch.nn.Parameter(torch.zeros(2, 4))
        g.Lu = torch.nn.Parameter(torch.eye(4).repeat(2, 1, 1))
        return g
    out = []
    for lik in ("poisson", "nb"):
        out += [NSF(gp(), y, L=2, likelihood=lik), NSF2(gp(), y, L=2, likelihood=lik),
                Hybrid_NSF(gp(), y, L=2, non_spatial_factors=2, likelihood=lik),
                Hybrid_NSF2(gp(), G.GaussianPrior(y, L=2), y, L=2, T=2, likelihood=lik)]
    return out, torch.zeros(9, 2), y


def test_family_and_theta_are_validated_before_anything_runs():
    """On CPU tensors: every refusal below comes before the first kernel would be asked for."""
    models, X, y = _cpu_models()
    for m in models:
        with pytest.raises(ValueError, match='"poisson", "nb" or "model"'):
            m.deviance(X, y, family="gamma")
        with pytest.raises(ValueError, match="belongs to family"):
            m.deviance(X, y, theta=3.0)
        with pytest.raises(ValueError, match="positive"):
            m.deviance(X, y, family="nb", theta=-1.0)
        with pytest.raises(ValueError, match="positive"):
            m.deviance(X, y, family="nb", theta=torch.tensor([1.0, 2.0, 0.0, 1.0, 1.0, 1.0]))
        with pytest.raises(ValueError, match="6 genes"):
            m.deviance(X, y, family="nb", theta=torch.ones(5))
        if m.likelihood == "poisson":
            with pytest.raises(ValueError, match="needs theta="):
                m.deviance(X, y, family="nb")
        # a valid request reaches the entry, which wants the GPU
        with pytest.raises(RuntimeError, match="GPU only"):
            m.deviance(X, y, family="nb", theta=2.0)
        if m.likelihood == "nb":
            with pytest.raises(RuntimeError, match="GPU only"):
                m.deviance(X, y, family="model")


def test_mggp_nsf_checks_groups_first_and_then_the_family():
    import gpzoo.gp as G
    import gpzoo.kernels as K
    from gpzoo.likelihoods import MGGP_NSF
    y = torch.ones(6, 9)
    k = K.MGGP_NSF_RBF(sigma=1.0, lengthscale=2.0, group_diff_param=0.8, n_groups=2, L=2)
    m = MGGP_NSF(G.MGGP_WSVGP(k, dim=2, M=4, n_groups=2, jitter=1e-2), y, L=2)
    with pytest.raises(TypeError, match="groupsX"):
        m.deviance(torch.zeros(9, 2), y, family="nb")
    with pytest.raises(ValueError, match="needs theta="):
        m.deviance(torch.zeros(9, 2), y, groupsX=torch.zeros(9, dtype=torch.long), family="nb")
    with pytest.raises(ValueError, match='"poisson", "nb" or "model"'):
        m.deviance(torch.zeros(9, 2), y, groupsX=torch.zeros(9, dtype=torch.long), family="NB")
