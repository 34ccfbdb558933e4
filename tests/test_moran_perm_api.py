"""CPU: the surface of the permutation null of Moran's I -- ``fdr_bh``, the argument checks of ``gene_autocorr(n_perms=)``,
the fields of ``GeneAutocorrPerm``, the C entries' declarations and bindings, their host-only plan queries and the argument
errors that come before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

NEW_SYMBOLS = ("gpz_gene_morans_perm_sparse", "gpz_gene_morans_perm_sparse_plan", "gpz_morans_perm_rows",
               "gpz_morans_perm_rows_plan")
OUTPUTS = ["I", "sims", "n_ge", "n_le", "sim_mean", "sim_m2", "info", "partials", "partials_bytes", "stream"]


def header():
    return open(os.path.join(ROOT, "include", "gpzoo_hip.h")).read()


def test_fdr_bh_against_a_hand_computed_vector():
    """m = 6 tests (the NaN is not one): sorted 0.001, 0.03, 0.03, 0.04, 0.5, 0.9 give m p / rank = 0.006, 0.09, 0.06, 0.06,
    0.6, 0.9, and the running minimum from the largest p 0.006, 0.06, 0.06, 0.06, 0.6, 0.9."""
    from gpzoo.utilities import fdr_bh
    p = torch.tensor([0.001, 0.04, float("nan"), 0.03, 0.03, 0.5, 0.9], dtype=torch.float64)
    want = np.array([0.006, 0.06, np.nan, 0.06, 0.06, 0.6, 0.9])
    got = fdr_bh(p)
    assert got.dtype == torch.float64 and got.shape == p.shape
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-15, atol=0, equal_nan=True)
    np.testing.assert_allclose(fdr_bh(p.float()).numpy(), want, rtol=1e-6, equal_nan=True)
    assert fdr_bh(torch.tensor([0.9, 0.95], dtype=torch.float64)).tolist() == [0.95, 0.95]
    assert fdr_bh(torch.tensor([2.0, 0.5], dtype=torch.float64)).tolist() == [1.0, 1.0]         # clipped at 1
    assert torch.isnan(fdr_bh(torch.tensor([float("nan")] * 3))).all() and fdr_bh(torch.zeros(0)).shape == (0,)
    with pytest.raises(ValueError):
        fdr_bh(torch.zeros(2, 2))
    with pytest.raises(ValueError):
        fdr_bh([0.1, 0.2])


def test_fields_of_the_result():
    from gpzoo.utilities import GeneAutocorr, GeneAutocorrPerm
    assert GeneAutocorr._fields == ("I", "expected", "variance", "z")
    assert GeneAutocorrPerm._fields == ("I", "expected", "variance", "z", "n_perms", "n_ge", "n_le", "pval_greater", "pval_less",
                                        "pval_sim", "mean_sim", "var_sim", "z_sim", "pval_z_sim", "sims")
    import gpzoo.utilities as U
    import gpzoo_amd.utilities as A
    for name in ("GeneAutocorrPerm", "fdr_bh", "gene_autocorr"):
        assert getattr(U, name) is getattr(A, name)


def test_argument_errors_of_gene_autocorr_come_before_any_device_work():
    from gpzoo.utilities import gene_autocorr
    D, N = 5, 9
    V = torch.rand(D, N)
    nbr = torch.stack([(torch.arange(N) + s) % N for s in (1, 2)], dim=1)
    good = torch.stack([torch.randperm(N) for _ in range(3)])
    for bad in (0, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="n_perms"):
            gene_autocorr(V, graph=nbr, n_perms=bad)
    for bad in (good[:, :-1], good[0], good.double(), good > 2, torch.zeros((0, N), dtype=torch.int64), good.numpy()[:, :4]):
        with pytest.raises(ValueError, match=r"perms must be a \(P, 9\) integer tensor"):
            gene_autocorr(V, graph=nbr, perms=bad)
    with pytest.raises(ValueError, match="exclude each other"):
        gene_autocorr(V, graph=nbr, n_perms=3, perms=good)
    import inspect
    sig = inspect.signature(gene_autocorr)
    assert [sig.parameters[k].default for k in ("n_perms", "seed", "perms", "return_sims")] == [None, 0, None, False]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("n_perms", "seed", "perms", "return_sims"))
    doc = " ".join(gene_autocorr.__doc__.split())
    assert "PySAL" in doc and "1 / (P + 1)" in doc and "rows of its adjacency matrix" in doc
    from gpzoo.utilities import dims_autocorr
    assert "gene_autocorr(factors.T, coords, n_perms=" in " ".join(dims_autocorr.__doc__.split())


def test_new_entries_are_declared_exported_and_bound():
    from gpzoo_amd import _lib, build, ops
    hdr = header()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in hdr and name in _lib.exported_symbols() and hasattr(lib, name)
    assert lib.gpz_version() == 212
    assert all(callable(getattr(ops, n)) for n in ("gene_morans_perm_sparse", "morans_perm_rows", "morans_perm_plan"))
    assert "moran_perm.hip" in build.SOURCES and "moran_expr.h" in build.HEADERS
    assert '#include "moran_expr.h"' in open(os.path.join(build.CSRC, "moran_perm.hip")).read()
    assert "-ffp-contract=off" in build.SOURCE_FLAGS["moran_perm.hip"]          # gene_rank.hip's expression, gene_rank.hip's bits
    assert "-ffp-contract=off" in build.SOURCE_FLAGS["gene_rank.hip"]


def _args(name):
    args = re.search(rf"\b{name}\s*\(([^;{{]*?)\)\s*;", header(), flags=re.S).group(1)
    return [a.split()[-1].lstrip("*") for a in args.replace("\n", " ").split(",")]


def test_scratch_is_the_explicit_argument_partials_sized_by_the_plan():
    hdr = header()
    assert _args("gpz_gene_morans_perm_sparse") == ["row_ptr", "row_spot", "row_perm", "col_val", "nbr", "perms", "N", "D", "nnz", "K",
                                                    "P", "perm_batch", "line_mode"] + OUTPUTS
    assert _args("gpz_morans_perm_rows") == ["values", "nbr", "perms", "N", "D", "K", "P", "perm_batch", "line_mode"] + OUTPUTS
    plan_outs = ["perm_batch", "line_mode", "workgroups", "partials_bytes"]
    assert _args("gpz_gene_morans_perm_sparse_plan") == ["N", "D", "nnz", "K", "P", "perm_batch_wanted", "line_mode_wanted"] + plan_outs
    assert _args("gpz_morans_perm_rows_plan") == ["N", "D", "K", "P", "perm_batch_wanted", "line_mode_wanted"] + plan_outs
    for name in NEW_SYMBOLS:
        assert "ws" not in _args(name) and f"{name}_workspace_bytes" not in hdr
    import scratch_cases as S
    assert not set(NEW_SYMBOLS) & S.header_entries_with_workspace(hdr)


def test_plan_queries_need_no_device():
    from gpzoo_amd import ops
    N, D, K, P = 39694, 17702, 6, 100
    sp = ops.morans_perm_plan(N, D, K, P, nnz=35_000_000)
    rows = ops.morans_perm_plan(N, D, K, P)
    # the line in LDS wherever it fits, then one permutation per wave of the workgroup; eight with the line in the scratch
    assert sp["line_mode"] == rows["line_mode"] == 2 and sp["perm_batch"] == rows["perm_batch"] == 16
    assert ops.morans_perm_plan(N, D, K, P, nnz=1, line_mode=1)["perm_batch"] == 8
    tables = sp["perm_batch"] * N * (K + 2) * 4
    lines = sp["workgroups"] * N * 4
    assert 1 <= sp["workgroups"] <= D
    assert tables + lines + N * 4 + D * 32 <= sp["partials_bytes"] <= tables + lines + N * 4 + D * 32 + 8 * 256
    assert abs(sp["partials_bytes"] - rows["partials_bytes"] - lines) <= 512                  # dense rows are their own lines
    assert ops.morans_perm_plan(N, D, K, 1000, nnz=1, perm_batch=32)["perm_batch"] == 32      # the LDS arrays of a batch
    # the tables of a batch, (K + 2) int32 per spot and permutation, take at most 256 MiB
    assert ops.morans_perm_plan(1 << 20, D, 32, 1000, nnz=1)["perm_batch"] == (256 << 20) // ((1 << 20) * 34 * 4) == 1
    assert ops.morans_perm_plan(1 << 19, D, 32, 1000, nnz=1)["perm_batch"] == 3
    assert ops.morans_perm_plan(1 << 28, D, 32, 1000, nnz=1)["perm_batch"] == 1
    assert ops.morans_perm_plan(N, D, K, 5, nnz=1)["perm_batch"] == 5
    assert ops.morans_perm_plan(N, D, K, 5, nnz=1, perm_batch=8)["perm_batch"] == 5
    assert ops.morans_perm_plan(N, D, K, 50, nnz=1, perm_batch=8)["perm_batch"] == 8
    assert ops.morans_perm_plan(N, 3, K, 5)["workgroups"] == 3
    # the LDS line: 4 N bytes and the 512 bytes of the batch arrays within a workgroup's 160 KiB
    fit = (160 * 1024 - 512) // 4
    assert fit == 40832 and N <= fit
    for mode in (2, "lds"):
        assert ops.morans_perm_plan(fit, D, K, P, line_mode=mode)["line_mode"] == 2
        assert ops.morans_perm_plan(N, D, K, P, nnz=10, line_mode=mode)["line_mode"] == 2
        with pytest.raises(ValueError, match="does not fit"):
            ops.morans_perm_plan(fit + 1, D, K, P, line_mode=mode)
    assert ops.morans_perm_plan(fit + 1, D, K, P)["line_mode"] == 1                           # auto never asks for what does not fit
    assert ops.morans_perm_plan(N, D, K, P, line_mode="global")["line_mode"] == 1
    for bad in (3, -1, "LDS", True, None):
        with pytest.raises(ValueError, match="line_mode"):
            ops.morans_perm_plan(N, D, K, P, line_mode=bad)
    for bad in (dict(P=0), dict(P=1 << 31), dict(perm_batch=33), dict(perm_batch=-1), dict(K=0), dict(K=33), dict(N=6), dict(D=0)):
        with pytest.raises(ValueError):
            ops.morans_perm_plan(**{**dict(N=N, D=D, K=K, P=P), **bad})
    with pytest.raises(ValueError, match="32 bits"):
        ops.morans_perm_plan(N, D, K, P, nnz=1 << 31)


def test_bad_arguments_are_refused_before_any_launch():
    from gpzoo_amd import _lib
    lib = _lib.load()
    # host memory stands in for device memory: every refusal below comes before the first launch
    buf = (C.c_char * 16384)()
    base = (C.addressof(buf) + 15) & ~15
    p = lambda off=0: C.c_void_p(base + off)  # noqa: E731
    ins = [p(256 * i) for i in range(6)]
    outs = [p(2048 + 256 * i) for i in range(7)]

    def sparse(ins=ins, N=10, D=4, nnz=5, K=6, P=3, pb=0, mode=0, outs=outs, scratch=p(8192), nbytes=1 << 30):
        return lib.gpz_gene_morans_perm_sparse(*ins, N, D, nnz, K, P, pb, mode, *outs, scratch, nbytes, None)

    def rows(ins=ins[:3], N=10, D=4, K=6, P=3, pb=0, mode=0, outs=outs, scratch=p(8192), nbytes=1 << 30):
        return lib.gpz_morans_perm_rows(*ins, N, D, K, P, pb, mode, *outs, scratch, nbytes, None)
    for f, who in ((sparse, b"gpz_gene_morans_perm_sparse"), (rows, b"gpz_morans_perm_rows")):
        assert f(ins=[None] + ins[1:6 if f is sparse else 3]) < 0 and who + b": null pointer" in lib.gpz_last_error()
        for i in (0, 2, 3, 4, 5, 6):                                  # every output but sims is needed
            assert f(outs=outs[:i] + [None] + outs[i + 1:]) < 0 and who + b": null pointer" in lib.gpz_last_error()
        assert f(scratch=None) < 0 and who + b": null pointer" in lib.gpz_last_error()
        assert f(N=0) < 0 and b"bad extents" in lib.gpz_last_error()
        assert f(D=1 << 31) < 0 and b"32 bits" in lib.gpz_last_error()
        for K in (0, 33, 10):
            assert f(K=K) < 0 and b"neighbours of N = 10 spots unsupported" in lib.gpz_last_error()
        assert f(P=0) < 0 and b"P = 0 permutations" in lib.gpz_last_error()
        assert f(pb=33) < 0 and b"perm_batch = 33" in lib.gpz_last_error()
        assert f(mode=3) < 0 and b"line_mode 3 unknown" in lib.gpz_last_error()
        assert f(N=50000, K=6, mode=2) < 0 and b"does not fit" in lib.gpz_last_error()
        assert f(scratch=p(8200)) < 0 and b"16-byte aligned" in lib.gpz_last_error()
        assert f(nbytes=64) < 0 and b"partials too small" in lib.gpz_last_error()
    assert sparse(ins=ins[:2] + [None] + ins[3:]) < 0 and b"null pointer (non-zeros)" in lib.gpz_last_error()
    assert sparse(nnz=1 << 31) < 0 and b"32 bits" in lib.gpz_last_error()


def test_ops_refuse_bad_arguments_without_a_device():
    from gpzoo.likelihoods import SparseCounts
    from gpzoo_amd import ops
    Y = torch.tensor(np.random.default_rng(0).poisson(0.7, size=(5, 9)).astype(np.float32))
    c = SparseCounts(Y)
    nbr = torch.stack([(torch.arange(9) + s) % 9 for s in (1, 2)], dim=1)
    perms = torch.stack([torch.randperm(9) for _ in range(3)]).to(torch.int32)
    with pytest.raises(TypeError):
        ops.gene_morans_perm_sparse(Y, nbr, perms)
    with pytest.raises(TypeError, match="view"):
        ops.gene_morans_perm_sparse(c[:, torch.arange(4)], nbr, perms)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.gene_morans_perm_sparse(c, nbr, perms)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.morans_perm_rows(Y, nbr, perms)
    with pytest.raises(ValueError, match="float32"):
        ops.morans_perm_rows(Y.double(), nbr, perms)
