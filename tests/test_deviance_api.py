"""CPU: the surface of the Poisson deviance -- the C ABI's new symbols and host-only queries, the argument checks that
return before any launch (through ctypes, with pointers that are never dereferenced), the Python names, and
train_val_split against the reference's anndata_to_train_val (fixtures written by tests/golden/make_trainval_golden.py
from the reference itself)."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import torch

from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpz_poisson_deviance", "gpz_poisson_deviance_workspace_bytes", "gpz_poisson_deviance_plan",
       "gpz_poisson_deviance_sparse", "gpz_poisson_deviance_sparse_workspace_bytes", "gpz_poisson_deviance_sparse_plan")


def test_new_symbols_are_bound_and_declared_under_version_212():
    from gpzoo_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "gpzoo_hip.h")).read()
    assert re.search(r"^#define GPZ_VERSION 212$", header, re.M)
    for name in NEW:
        assert name in _lib.exported_symbols(), name
        assert re.search(r"\b%s\(" % name, header), name
    assert "deviance.hip" in build.SOURCES


def test_plan_queries_answer_without_a_device():
    from gpzoo_amd import ops
    p = ops.poisson_deviance_plan(7000, 17702, 20)
    assert p["spots_per_tile"] > 0 and p["genes_per_tile"] > 0 and p["genes_per_block"] % p["genes_per_tile"] == 0
    assert p["gene_slices"] == -(-17702 // p["genes_per_block"]) and p["factors_padded"] >= 20 and p["workspace_bytes"] > 0
    assert p["spot_slices"] * p["tiles_per_spot_slice"] >= -(-7000 // p["spots_per_tile"])
    s = ops.poisson_deviance_sparse_plan(39694, 7000, 17702, 20, 35_000_000)
    assert s["gene_chunk"] > 0 and s["n_gene_chunks"] >= 17702 and s["factors_padded"] >= 20
    # no array of D x B or D x N elements, and nothing of nnz elements: the workspace is far below 4 bytes per non-zero
    assert s["workspace_bytes"] < 35_000_000 and s["workspace_bytes"] < 17702 * 7000
    for bad in (0, 65):
        with pytest.raises(ValueError, match="factors"):
            ops.poisson_deviance_plan(100, 50, bad)
        with pytest.raises(ValueError, match="factors"):
            ops.poisson_deviance_sparse_plan(100, 100, 50, bad, 10)


def _fake(n=1):
    """Aligned non-null addresses for arguments the entries check and never dereference on the host."""
    return [C.c_void_p(0x10000 * (i + 1)) for i in range(n)]


def test_dense_argument_errors_return_before_any_launch():
    from gpzoo_amd import _lib
    lib = _lib.load()
    N, D, Lt = 130, 80, 5
    need = lib.gpz_poisson_deviance_workspace_bytes(N, D, Lt)
    assert need > 0

    def call(ptrs=None, Lt=Lt, ws=C.c_void_p(0x900000), ws_bytes=need):
        p = _fake(9) if ptrs is None else ptrs
        return lib.gpz_poisson_deviance(*p[:5], N, D, Lt, 1, *p[5:9], ws, ws_bytes, None)

    def refused(rc, word):
        assert rc == -1
        assert word in lib.gpz_last_error().decode()

    refused(call(Lt=0), "factors")
    refused(call(Lt=65), "factors")
    assert lib.gpz_poisson_deviance_workspace_bytes(N, D, 0) == 0 and lib.gpz_poisson_deviance_workspace_bytes(N, D, 65) == 0
    assert lib.gpz_poisson_deviance_workspace_bytes(0, D, Lt) == 0
    for k in range(9):
        p = _fake(9)
        p[k] = None
        refused(call(ptrs=p), "null pointer")
    refused(call(ws=None), "null pointer")
    refused(call(ws_bytes=need - 1), "workspace")
    p = _fake(9)
    p[2] = C.c_void_p(0x30004)                       # W
    refused(call(ptrs=p), "aligned")
    refused(call(ws=C.c_void_p(0x900008)), "aligned")


def test_sparse_argument_errors_return_before_any_launch():
    from gpzoo_amd import _lib
    lib = _lib.load()
    N, B, D, Lt, nnz = 130, 37, 80, 5, 900
    need = lib.gpz_poisson_deviance_sparse_workspace_bytes(N, B, D, nnz, Lt)
    assert need > 0

    def call(ptrs=None, B=B, Lt=Lt, ws=C.c_void_p(0x900000), ws_bytes=need, nnz=nnz):
        p = _fake(16) if ptrs is None else ptrs
        return lib.gpz_poisson_deviance_sparse(*p[:12], N, B, D, nnz, Lt, 1, *p[12:16], ws, ws_bytes, None)

    def refused(rc, word):
        assert rc == -1
        assert word in lib.gpz_last_error().decode()

    refused(call(Lt=0), "factors")
    refused(call(Lt=65), "factors")
    assert lib.gpz_poisson_deviance_sparse_workspace_bytes(N, B, D, nnz, 65) == 0
    assert lib.gpz_poisson_deviance_sparse_workspace_bytes(N, N + 1, D, nnz, Lt) == 0
    for k in (0, 1, 2, 3, 4, 7, 12, 13, 14, 15):
        p = _fake(16)
        p[k] = None
        refused(call(ptrs=p), "null pointer")
    p = _fake(16)
    p[5] = None                                      # col_gene with nnz > 0
    refused(call(ptrs=p), "null pointer")
    p = _fake(16)
    p[10] = None                                     # idx without pos
    refused(call(ptrs=p), "idx and pos")
    p = _fake(16)
    p[10] = p[11] = None                             # no view, but B < N
    refused(call(ptrs=p), "needs idx and pos")
    refused(call(ws=None), "null pointer")
    refused(call(ws_bytes=need - 1), "workspace")
    p = _fake(16)
    p[2] = C.c_void_p(0x30004)
    refused(call(ptrs=p), "aligned")
    refused(call(ws=C.c_void_p(0x900008)), "aligned")


def test_python_names_resolve_through_the_shims():
    import gpzoo.likelihoods as L
    import gpzoo.utilities as U
    import gpzoo_amd.likelihoods as AL
    import gpzoo_amd.utilities as AU
    from gpzoo_amd import ops
    assert L.poisson_deviance is AL.poisson_deviance and L.PoissonDeviance is AL.PoissonDeviance
    assert U.train_val_split is AU.train_val_split
    assert AL.PoissonDeviance._fields == ("total", "mean", "per_gene", "per_spot", "null_total", "null_per_gene", "explained",
                                          "explained_per_gene", "sum_y", "sum_mu")
    for cls in ("NSF", "NSF2", "MGGP_NSF", "Hybrid_NSF2", "Hybrid_NSF_Exact", "Hybrid_NSF"):
        assert callable(getattr(getattr(L, cls), "deviance")), cls
    assert callable(ops.poisson_deviance) and callable(ops.poisson_deviance_sparse)
    assert "anndata_to_train_val" in AU._NOT_REBUILT
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.poisson_deviance(torch.zeros(2, 3), torch.ones(2, 3), torch.ones(4, 2), torch.ones(3), torch.ones(4, 3))


FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "extra_trainval_*.npz")))


def test_trainval_fixtures_exist():
    assert len(FIXTURES) == 6


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[len("extra_trainval_"):-4] for p in FIXTURES])
@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_train_val_split_matches_the_reference(path, form):
    from gpzoo_amd.likelihoods import SparseCounts
    from gpzoo_amd.utilities import train_val_split
    z = np.load(path, allow_pickle=False)
    sz = os.path.basename(path).split("_")[2]
    coords = torch.from_numpy(z["coords"])
    y = torch.from_numpy(z["Y"].T.copy()).float()                   # genes x spots
    counts = SparseCounts(y) if form == "sparse" else y
    Dtr, Dval = train_val_split(coords, counts, train_frac=float(z["train_frac"]), sz=sz)
    assert (Dval is not None) == bool(z["has_val"])
    start = 0
    for tag, d in (("tr", Dtr), ("val", Dval)):
        if d is None:
            continue
        want_Y = torch.from_numpy(z[f"{tag}_Y"]).double()
        n = want_Y.shape[0]
        idx = torch.arange(start, start + n)
        assert torch.equal(d["idx"], idx)
        if f"{tag}_idx" in z:                                        # the reference sets it for the training part
            assert np.array_equal(z[f"{tag}_idx"], d["idx"].numpy())
        got_y = d["y"].to_dense() if form == "sparse" else d["y"]
        if form == "sparse":
            assert isinstance(d["y"], SparseCounts) and d["y"].base is d["y"] and d["y"].shape == (y.shape[0], n)
        assert torch.equal(got_y.double(), want_Y.T)
        assert d["sz"].shape == (n,)
        torch.testing.assert_close(d["sz"].double(), torch.from_numpy(z[f"{tag}_sz"]).double().reshape(-1), rtol=1e-6, atol=0.0,
                                   equal_nan=True)
        assert torch.equal(d["X"], coords[idx])                      # rows by index; not rescaled here
        start += n


def test_train_val_split_refuses_what_it_cannot_split():
    from gpzoo_amd.likelihoods import SparseCounts
    from gpzoo_amd.utilities import train_val_split
    y = torch.ones(3, 10)
    with pytest.raises(ValueError, match="unrecognized size factors"):
        train_val_split(torch.zeros(10, 2), y, sz="median")
    with pytest.raises(ValueError, match="rows of X"):
        train_val_split(torch.zeros(9, 2), y)
    with pytest.raises(TypeError, match="view"):
        train_val_split(torch.zeros(4, 2), SparseCounts(y)[:, torch.arange(4)])
    Dtr, Dval = train_val_split(torch.zeros(10, 2), y, train_frac=0.95)
    assert Dtr["y"].shape == (3, 10) and Dval is None
