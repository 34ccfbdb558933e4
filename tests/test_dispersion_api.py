"""CPU: the surface of the gene-wise dispersion fit -- the C entries' declarations, bindings and host-side refusals, the plan
query, the refusals of ``gene_dispersion`` / ``rank_genes(by="overdispersion")`` before any device work, per-gene ``theta0``
arrays on every count model, and the re-exports under the ``gpzoo`` names."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_nb_api import COUNT_MODELS, D, builders, reference_keys

NEW_SYMBOLS = ("gpz_gene_dispersion_sparse", "gpz_gene_dispersion_sparse_plan")


def header():
    return open(os.path.join(ROOT, "include", "gpzoo_hip.h")).read()


def _args(name):
    args = re.search(rf"\b{name}\s*\(([^;{{]*?)\)\s*;", header(), flags=re.S).group(1)
    return [a.split()[-1].lstrip("*") for a in args.replace("\n", " ").split(",")]


def test_new_entries_are_declared_exported_and_bound():
    from gpzoo_amd import _lib, build, ops
    hdr = header()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in hdr and name in _lib.exported_symbols()
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
    assert lib.gpz_version() == 212 and "#define GPZ_VERSION 212" in hdr
    comment = hdr[hdr.index("Additions under version 212"):hdr.index("#ifndef GPZOO_HIP_H")]
    assert "gpz_gene_dispersion_sparse" in comment and "gpz_gene_dispersion_sparse_plan" in comment
    assert callable(ops.gene_dispersion_sparse) and callable(ops.gene_dispersion_plan)
    assert "gene_dispersion.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "gene_dispersion.hip"))
    assert "-ffp-contract=off" in build.SOURCE_FLAGS["gene_dispersion.hip"]
    # the row helpers live in one header, which both sources include and the source hash covers
    assert "gene_rows.h" in build.HEADERS
    for src in ("gene_rank.hip", "gene_dispersion.hip"):
        text = open(os.path.join(build.CSRC, src)).read()
        assert '#include "gene_rows.h"' in text and "struct GrRows" not in text and "void gr_tree" not in text


def test_scratch_is_the_explicit_argument_partials_sized_by_the_plan():
    hdr = header()
    assert _args("gpz_gene_dispersion_sparse") == [
        "row_ptr", "row_spot", "row_perm", "col_val", "size", "N", "D", "nnz", "theta_min", "theta_max", "max_iter", "theta", "gain",
        "poisson_loglik", "status", "iterations", "info", "partials", "partials_bytes", "stream"]
    assert _args("gpz_gene_dispersion_sparse_plan") == ["N", "D", "nnz", "gene_chunk", "workgroups", "tol_t", "partials_bytes"]
    assert "ws" not in _args("gpz_gene_dispersion_sparse") and "ws_bytes" not in _args("gpz_gene_dispersion_sparse")
    assert "gpz_gene_dispersion_sparse_workspace_bytes" not in hdr
    import scratch_cases as S
    assert not set(NEW_SYMBOLS) & S.header_entries_with_workspace(hdr)


def test_plan_query_needs_no_device():
    from gpzoo_amd import ops
    p = ops.gene_dispersion_plan(39694, 17702, 35_000_000)
    assert set(p) == {"gene_chunk", "workgroups", "tol_t", "partials_bytes"}
    assert p["gene_chunk"] == ops.gene_rank_plan(39694, 17702, 35_000_000)["gene_chunk"] and p["gene_chunk"] % 64 == 0
    assert 1 <= p["workgroups"] <= 17702 and 0 < p["tol_t"] <= 1e-9 and 0 < p["partials_bytes"] <= 4096
    # nothing of D x N or nnz elements: the scratch does not depend on the shape beyond the workgroups
    for shape in ((39694, 10 * 17702, 1), (7, 17702, 35_000_000), (4099, 3, 10)):
        assert ops.gene_dispersion_plan(*shape)["partials_bytes"] == p["partials_bytes"]
    assert ops.gene_dispersion_plan(4099, 3, 10)["workgroups"] == 3
    for bad in ((0, 1, 0), (5, 1, 1 << 31), (5, 0, 0), (1 << 31, 1, 0)):
        with pytest.raises(ValueError):
            ops.gene_dispersion_plan(*bad)


def test_bad_arguments_are_refused_before_any_launch():
    from gpzoo_amd import _lib
    lib = _lib.load()
    who = b"gpz_gene_dispersion_sparse: "
    assert lib.gpz_gene_dispersion_sparse(*([None] * 5), 10, 4, 5, 1e-4, 1e6, 50, *([None] * 7), 0, None) < 0
    assert who + b"null pointer" in lib.gpz_last_error()
    # host memory stands in for device memory: every refusal below comes before the first launch
    buf = (C.c_char * 8192)()
    base = (C.addressof(buf) + 15) & ~15
    p = lambda off=0: C.c_void_p(base + off)  # noqa: E731
    ok = [p(256 * i) for i in range(5)]
    outs = [p(2048 + 256 * i) for i in range(6)]

    def run(inputs=ok, N=10, D=4, nnz=5, lo=1e-4, hi=1e6, max_iter=50, outs=outs, scratch=p(4096), nbytes=1 << 20):
        return lib.gpz_gene_dispersion_sparse(*inputs, N, D, nnz, lo, hi, max_iter, *outs, scratch, nbytes, None)
    for i in range(6):
        assert run(outs=outs[:i] + [None] + outs[i + 1:]) < 0 and who + b"null pointer" in lib.gpz_last_error()
    assert run(inputs=[None] + ok[1:]) < 0 and who + b"null pointer" in lib.gpz_last_error()
    assert run(inputs=ok[:4] + [None]) < 0 and who + b"null pointer" in lib.gpz_last_error()
    assert run(inputs=[ok[0], None] + ok[2:]) < 0 and b"null pointer (non-zeros)" in lib.gpz_last_error()
    assert run(scratch=None) < 0 and who + b"null pointer" in lib.gpz_last_error()
    assert run(N=0) < 0 and b"bad extents" in lib.gpz_last_error()
    assert run(D=0) < 0 and b"bad extents" in lib.gpz_last_error()
    assert run(nnz=-1) < 0 and b"bad extents" in lib.gpz_last_error()
    assert run(nnz=1 << 31) < 0 and b"32 bits" in lib.gpz_last_error()
    for lo, hi in ((0.0, 1.0), (-1.0, 1.0), (2.0, 2.0), (3.0, 2.0), (1.0, float("inf")), (float("nan"), 1.0), (1.0, float("nan"))):
        assert run(lo=lo, hi=hi) < 0 and b"theta range" in lib.gpz_last_error(), (lo, hi)
    for it in (-1, 201, 1 << 20):
        assert run(max_iter=it) < 0 and b"outside [0, 200]" in lib.gpz_last_error()
    assert run(scratch=p(4100)) < 0 and b"16-byte aligned" in lib.gpz_last_error()
    assert run(nbytes=8) < 0 and b"partials too small" in lib.gpz_last_error()


def _counts():
    from gpzoo.likelihoods import SparseCounts
    Y = np.random.default_rng(0).poisson(0.7, size=(9, 13)).astype(np.float32)
    Y[4] = 0
    return SparseCounts(torch.tensor(Y))


def test_refusals_come_before_any_device_work():
    from gpzoo import utilities as ut
    from gpzoo_amd import ops
    y = _counts()
    e = ut.log_normalize(y)
    view = y[:, torch.tensor([0, 2])]
    with pytest.raises(TypeError, match="not counts"):
        ut.gene_dispersion(e)
    for bad in (y.T, view, y.to_dense(), np.zeros((3, 4))):
        with pytest.raises(TypeError):
            ut.gene_dispersion(bad)
        with pytest.raises(TypeError):
            ut.rank_genes(bad, by="overdispersion")
        with pytest.raises(TypeError):
            ops.gene_dispersion_sparse(bad, torch.ones(13, dtype=torch.float64))
    with pytest.raises(TypeError):
        ut.rank_genes(e, by="overdispersion")
    for rng in ((0.0, 1.0), (2.0, 1.0), (1.0, 1.0), (1.0, float("inf")), (float("nan"), 2.0), (1.0,), "ab", 3.0):
        with pytest.raises(ValueError, match="theta_range"):
            ut.gene_dispersion(y, theta_range=rng)
    with pytest.raises(ValueError, match="size_factors"):
        ut.gene_dispersion(y, np.ones(12))
    with pytest.raises(ValueError, match="positive"):
        ut.gene_dispersion(y, size_factors=np.zeros(13))
    with pytest.raises(ValueError, match="positive"):
        ut.gene_dispersion(y, size_factors=np.full(13, np.inf))
    for it in (-1, 201, 2.5):
        with pytest.raises(ValueError, match="max_iter"):
            ut.gene_dispersion(y, max_iter=it)
    with pytest.raises(ValueError, match="float64"):
        ops.gene_dispersion_sparse(y, torch.ones(13))
    with pytest.raises(ValueError, match="theta range"):
        ops.gene_dispersion_sparse(y, torch.ones(13, dtype=torch.float64), 1.0, 0.5)
    with pytest.raises(RuntimeError, match="GPU only"):          # whole CPU counts pass every check and stop at the device
        ut.gene_dispersion(y)
    with pytest.raises(RuntimeError, match="GPU only"):
        ut.rank_genes(y, by="overdispersion")
    with pytest.raises(ValueError, match="by="):                 # unchanged
        ut.rank_genes(y, by="variance")
    with pytest.raises(ValueError, match="family"):
        ut.gene_deviance(y, family="nb")


def _softplus(m):
    return torch.nn.functional.softplus(m.theta.detach().double())


@pytest.mark.parametrize("name", COUNT_MODELS)
def test_theta0_takes_one_value_per_gene(name):
    start = np.exp(np.linspace(np.log(1e-2), np.log(1e3), D))
    for given in (start, torch.tensor(start), torch.tensor(start, dtype=torch.float32), list(start)):
        m = builders(likelihood="nb", theta0=given)[name]()
        assert isinstance(m.theta, torch.nn.Parameter) and m.theta.shape == (D,) and m.theta.dtype == torch.get_default_dtype()
        torch.testing.assert_close(_softplus(m), torch.tensor(start), rtol=1e-5, atol=1.1e-5)      # init_softplus floors by 1e-5
        assert set(m.state_dict()) == set(reference_keys()[name]) | {"theta"}
    for bad in (start[:-1], start.reshape(1, D), np.ones((D, 1)), torch.ones(D + 1), []):
        with pytest.raises(ValueError, match="theta0"):
            builders(likelihood="nb", theta0=bad)[name]()
    for value in (0.0, -1.0, np.nan, np.inf):
        bad = start.copy()
        bad[3] = value
        with pytest.raises(ValueError, match="theta0"):
            builders(likelihood="nb", theta0=bad)[name]()
        with pytest.raises(ValueError, match="theta0"):
            builders(likelihood="nb", theta0=torch.tensor(bad))[name]()
    assert not hasattr(builders(theta0=start)[name](), "theta")     # Poisson ignores it, as it ignores the number


@pytest.mark.parametrize("name", COUNT_MODELS)
def test_scalar_theta0_gives_the_same_bits_as_before(name):
    from gpzoo.utilities import init_softplus
    for value, kw in ((10.0, {}), (3.5, dict(theta0=3.5)), (2.0, dict(theta0=torch.tensor(2.0))), (7.0, dict(theta0=np.float32(7.0)))):
        m = builders(likelihood="nb", **kw)[name]()
        want = torch.as_tensor(init_softplus(np.full((D,), float(value), dtype=np.float64)), dtype=torch.get_default_dtype())
        assert torch.equal(m.theta.detach(), want)
        same = builders(likelihood="nb", theta0=np.full(D, float(value)))[name]()
        assert torch.equal(same.theta.detach(), want)
    with pytest.raises(ValueError, match="theta0 must be positive"):
        builders(likelihood="nb", theta0=0.0)[name]()


def test_the_docstring_shows_the_start_from_a_fit():
    import gpzoo.likelihoods as li
    doc = " ".join(li._init_likelihood.__doc__.split())
    assert "theta0=disp.theta.nan_to_num(nan=10.0).clamp(1e-2, 1e3)" in doc and "lower-biased" in doc


def test_reexports_under_the_gpzoo_names():
    import gpzoo.utilities as ut
    import gpzoo_amd.utilities as aut
    for name in ("gene_dispersion", "GeneDispersion", "rank_genes"):
        assert getattr(ut, name) is getattr(aut, name)
    assert ut.GeneDispersion._fields == ("theta", "loglik", "poisson_loglik", "lr", "pvalue", "status", "iterations")
    sig = inspect.signature(ut.gene_dispersion)
    assert list(sig.parameters) == ["counts", "size_factors", "theta_range", "max_iter"]
    assert sig.parameters["size_factors"].default is None and sig.parameters["max_iter"].default == 50
    assert sig.parameters["theta_range"].default == (1e-4, 1e6)
    assert sig.parameters["theta_range"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "overdispersion" in ut.rank_genes.__doc__
