"""CPU: the surface of gene ranking and selection -- ``select_genes`` against the dense construction, every refusal, the
ordering rules of ``rank_genes``, the C entries' declarations, bindings and host-side argument checks, and the re-exports
under the ``gpzoo`` names."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

NEW_SYMBOLS = ("gpz_gene_deviance_sparse", "gpz_gene_deviance_sparse_plan", "gpz_gene_morans_i_sparse",
               "gpz_gene_morans_i_sparse_plan")
PARTS = ("col_ptr", "col_gene", "col_val", "row_ptr", "row_spot", "row_perm")


def header():
    return open(os.path.join(ROOT, "include", "gpzoo_hip.h")).read()


def _dense(seed=0, D=9, N=13):
    rng = np.random.default_rng(seed)
    Y = rng.poisson(0.7, size=(D, N)).astype(np.float32)
    Y[4] = 0                                                      # a gene with no entries
    return torch.tensor(Y)


def _same(a, b):
    assert tuple(a.shape) == tuple(b.shape)
    for k in PARTS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and torch.equal(x, y), k
    assert a.base is a and a.idx is None and a.pos is None


GENE_LISTS = {
    "permutation": [8, 0, 3, 4, 7, 1, 2, 6, 5],
    "single": [6],
    "all": list(range(9)),
    "empty-gene": [4, 2],
    "subset": [7, 4, 0],
}


@pytest.mark.parametrize("name", list(GENE_LISTS))
def test_select_genes_equals_the_dense_construction(name):
    from gpzoo.likelihoods import SparseCounts
    Y = _dense()
    y = SparseCounts(Y)
    genes = GENE_LISTS[name]
    want = SparseCounts(Y[genes])
    for g in (genes, torch.tensor(genes), torch.tensor(genes, dtype=torch.int32), np.array(genes), tuple(genes)):
        got = y.select_genes(g)
        _same(got, want)
        assert torch.equal(got.to_dense(), Y[genes])
    assert tuple(y.shape) == (9, 13) and torch.equal(y.to_dense(), Y)         # the source is untouched


def test_select_genes_of_an_input_that_needed_duplicate_summing():
    from gpzoo.likelihoods import SparseCounts
    ind = torch.tensor([[0, 0, 2, 2, 2, 1, 3], [1, 1, 0, 4, 4, 2, 3]])
    coo = torch.sparse_coo_tensor(ind, torch.tensor([1.0, 2.0, 5.0, 1.0, 1.0, 0.0, 4.0]), (4, 5))
    y = SparseCounts(coo)
    dense = y.to_dense()
    assert dense[0, 1] == 3 and dense[2, 4] == 2 and y.nnz == 4
    _same(y.select_genes([2, 3, 0]), SparseCounts(dense[[2, 3, 0]]))


def test_select_genes_of_an_expression_carries_values_and_offset():
    from gpzoo.likelihoods import SparseCounts, SparseExpression
    from gpzoo.utilities import log_normalize
    Y = _dense(3)
    e = log_normalize(SparseCounts(Y))
    for genes in GENE_LISTS.values():
        got = e.select_genes(genes)
        assert isinstance(got, SparseExpression) and not got.is_view and tuple(got.shape) == (len(genes), 13)
        assert torch.equal(got.offset, e.offset[genes]) and got.offset.dtype == torch.float64
        # the values are real numbers: they are carried over bit for bit, in the order of the dense construction
        want = SparseCounts(e.values.to_dense()[genes])
        _same(got.values, want)
        assert torch.equal(got.to_dense(), e.to_dense()[genes])


def test_select_genes_refusals():
    from gpzoo.likelihoods import SparseCounts
    from gpzoo.utilities import log_normalize
    y = SparseCounts(_dense())
    e = log_normalize(y)
    for obj in (y, e):
        for bad in ([1, 1], [0, 9], [-1], [], list(range(9)) + [0], torch.tensor([2, 5, 2])):
            with pytest.raises(IndexError):
                obj.select_genes(bad)
        for bad in (torch.tensor([0.0, 1.0]), torch.tensor([True, False]), "abc", y):
            with pytest.raises(TypeError):
                obj.select_genes(bad)
        with pytest.raises(ValueError):
            obj.select_genes(torch.tensor([[0, 1]]))
        with pytest.raises(TypeError, match="view"):
            obj[:, torch.tensor([0, 2])].select_genes([0])


def test_scorers_refuse_wrong_inputs_before_any_device_work():
    from gpzoo.likelihoods import SparseCounts
    from gpzoo import utilities as ut
    y = SparseCounts(_dense())
    e = ut.log_normalize(y)
    view = y[:, torch.tensor([0, 2])]
    with pytest.raises(TypeError, match="not counts"):           # the wording of _counts_expected
        ut.gene_deviance(e)
    for bad in (y.T, view, _dense(), np.zeros((3, 4))):
        with pytest.raises(TypeError):
            ut.gene_deviance(bad)
    with pytest.raises(ValueError, match="family"):
        ut.gene_deviance(y, family="nb")
    with pytest.raises(ValueError, match="binomial"):
        ut.gene_deviance(y, family="binomial", size_factors=np.ones(13))
    with pytest.raises(ValueError, match="size_factors"):
        ut.gene_deviance(y, size_factors=np.ones(12))
    with pytest.raises(ValueError, match="positive"):
        ut.gene_deviance(y, size_factors=np.zeros(13))
    coords = np.random.default_rng(0).random((13, 2))
    for bad in (y.T, view, e[:, torch.tensor([0, 2])], [[1.0]]):
        with pytest.raises(TypeError):
            ut.gene_autocorr(bad, coords)
    with pytest.raises(ValueError):
        ut.gene_autocorr(y)                                      # neither coords nor graph
    with pytest.raises(ValueError):
        ut.gene_autocorr(y, coords[:5])
    with pytest.raises(ValueError):
        ut.gene_autocorr(y, graph=torch.zeros((13, 33), dtype=torch.int64))
    with pytest.raises(ValueError):
        ut.gene_autocorr(y, graph=torch.zeros((13, 2)))
    with pytest.raises(ValueError, match="by="):
        ut.rank_genes(y, by="variance")
    with pytest.raises(ValueError, match="coords"):
        ut.rank_genes(y, by="moran")
    for bad in (e, y.T, view):
        for by in ("deviance", "binomial_deviance", "moran"):
            with pytest.raises(TypeError):
                ut.rank_genes(bad, by=by, coords=coords)
    with pytest.raises(RuntimeError, match="GPU only"):          # whole CPU counts pass every check and stop at the device
        ut.gene_deviance(y)


def test_rank_order_rules_on_a_hand_made_score():
    from gpzoo.utilities import _rank_order
    nan = float("nan")
    s = torch.tensor([1.0, nan, 3.0, 1.0, -2.0, 3.0, nan, 0.0, float("inf"), -0.0], dtype=torch.float64)
    order = _rank_order(s)
    assert order.dtype == torch.int64
    assert order.tolist() == [8, 2, 5, 0, 3, 7, 9, 4, 1, 6]       # decreasing, ties in gene order, NaN last in gene order
    assert _rank_order(s, 3).tolist() == [8, 2, 5] and _rank_order(s, 10).tolist() == order.tolist()
    idx = np.argsort(-s.numpy(), kind="stable")                  # the rule of dims_autocorr(sort=True)
    assert order.tolist() == idx.tolist()
    for bad in (0, 11, -1):
        with pytest.raises(ValueError, match="nfeat"):
            _rank_order(s, bad)


def test_new_entries_are_declared_exported_and_bound():
    from gpzoo_amd import _lib, build, ops
    hdr = header()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in hdr and name in _lib.exported_symbols()
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
    assert lib.gpz_version() == 212 and "#define GPZ_VERSION 212" in hdr
    comment = hdr[hdr.index("Additions under version 212"):hdr.index("#ifndef GPZOO_HIP_H")]
    assert "gpz_gene_deviance_sparse" in comment and "gpz_gene_morans_i_sparse" in comment
    assert all(callable(getattr(ops, n)) for n in ("gene_deviance_sparse", "gene_morans_i_sparse", "gene_rank_plan"))
    assert "gene_rank.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "gene_rank.hip"))
    assert "-ffp-contract=off" in build.SOURCE_FLAGS["gene_rank.hip"]


def _args(name):
    args = re.search(rf"\b{name}\s*\(([^;{{]*?)\)\s*;", header(), flags=re.S).group(1)
    return [a.split()[-1].lstrip("*") for a in args.replace("\n", " ").split(",")]


def test_scratch_is_the_explicit_argument_partials_sized_by_the_plan():
    hdr = header()
    assert _args("gpz_gene_deviance_sparse") == ["row_ptr", "row_spot", "row_perm", "col_val", "size", "N", "D", "nnz", "family",
                                                 "sum", "count", "deviance", "partials", "partials_bytes", "stream"]
    assert _args("gpz_gene_morans_i_sparse") == ["row_ptr", "row_spot", "row_perm", "col_val", "nbr", "N", "D", "nnz", "K", "I",
                                                 "info", "partials", "partials_bytes", "stream"]
    assert _args("gpz_gene_deviance_sparse_plan") == ["N", "D", "nnz", "gene_chunk", "workgroups", "partials_bytes"]
    assert _args("gpz_gene_morans_i_sparse_plan") == ["N", "D", "nnz", "K", "gene_chunk", "workgroups", "partials_bytes"]
    for name in ("gpz_gene_deviance_sparse", "gpz_gene_morans_i_sparse"):
        assert "ws" not in _args(name) and "ws_bytes" not in _args(name)
        assert f"{name}_workspace_bytes" not in hdr
    import scratch_cases as S
    assert not set(NEW_SYMBOLS) & S.header_entries_with_workspace(hdr)


def test_plan_queries_need_no_device():
    from gpzoo_amd import ops
    dev = ops.gene_rank_plan(39694, 17702, 35_000_000)
    mor = ops.gene_rank_plan(39694, 17702, 35_000_000, K=6)
    assert dev["gene_chunk"] == mor["gene_chunk"] and dev["gene_chunk"] % 64 == 0
    assert 1 <= mor["workgroups"] <= 17702 and 0 < dev["partials_bytes"] <= 4096
    # the Moran scratch: one line of N floats per workgroup plus the in-degree, independent of D and of nnz
    assert mor["workgroups"] * 39694 * 4 <= mor["partials_bytes"] <= (mor["workgroups"] + 1) * 39694 * 4 + 1024
    assert ops.gene_rank_plan(39694, 10 * 17702, 1, K=6)["partials_bytes"] == mor["partials_bytes"]
    assert ops.gene_rank_plan(39694, 3, 10, K=6)["workgroups"] == 3
    for bad in (dict(N=0, D=1, nnz=0), dict(N=5, D=1, nnz=1 << 31), dict(N=5, D=0, nnz=0)):
        with pytest.raises(ValueError):
            ops.gene_rank_plan(**bad)
    for K in (0, 33, 5, 7):
        with pytest.raises(ValueError, match="K = "):
            ops.gene_rank_plan(5, 2, 3, K=K)


def test_bad_arguments_are_refused_before_any_launch():
    from gpzoo_amd import _lib
    lib = _lib.load()
    assert lib.gpz_gene_deviance_sparse(*([None] * 5), 10, 4, 5, 0, None, None, None, None, 0, None) < 0
    assert b"gpz_gene_deviance_sparse: null pointer" in lib.gpz_last_error()
    assert lib.gpz_gene_morans_i_sparse(*([None] * 5), 10, 4, 5, 6, None, None, None, 0, None) < 0
    assert b"gpz_gene_morans_i_sparse: null pointer" in lib.gpz_last_error()
    # host memory stands in for device memory: every refusal below comes before the first launch
    buf = (C.c_char * 8192)()
    base = (C.addressof(buf) + 15) & ~15
    p = lambda off=0: C.c_void_p(base + off)  # noqa: E731
    ok = [p(256 * i) for i in range(5)]
    outs = [p(2048), p(2304), p(2560)]

    def dev(inputs=ok, N=10, D=4, nnz=5, family=0, outs=outs, scratch=p(4096), nbytes=1 << 20):
        return lib.gpz_gene_deviance_sparse(*inputs, N, D, nnz, family, *outs, scratch, nbytes, None)

    def mor(inputs=ok, N=10, D=4, nnz=5, K=6, I=p(2048), info=p(2304), scratch=p(4096), nbytes=1 << 20):
        return lib.gpz_gene_morans_i_sparse(*inputs, N, D, nnz, K, I, info, scratch, nbytes, None)
    assert dev(family=2) < 0 and b"family 2 unknown" in lib.gpz_last_error()
    assert dev(N=0) < 0 and b"bad extents" in lib.gpz_last_error()
    assert dev(nnz=1 << 31) < 0 and b"32 bits" in lib.gpz_last_error()
    assert dev(inputs=[ok[0], None] + ok[2:]) < 0 and b"null pointer (non-zeros)" in lib.gpz_last_error()
    assert dev(outs=[p(2048), None, p(2560)]) < 0 and b"null pointer" in lib.gpz_last_error()
    assert dev(scratch=p(4100)) < 0 and b"16-byte aligned" in lib.gpz_last_error()
    assert dev(nbytes=4) < 0 and b"partials too small" in lib.gpz_last_error()
    for K in (0, 33, 10):
        assert mor(K=K) < 0 and b"neighbours of N = 10 spots unsupported" in lib.gpz_last_error()
    assert mor(D=1 << 31) < 0 and b"32 bits" in lib.gpz_last_error()
    assert mor(info=None) < 0 and b"null pointer" in lib.gpz_last_error()
    assert mor(inputs=ok[:3] + [None, ok[4]]) < 0 and b"null pointer (non-zeros)" in lib.gpz_last_error()
    assert mor(scratch=p(4104)) < 0 and b"16-byte aligned" in lib.gpz_last_error()
    assert mor(nbytes=64) < 0 and b"partials too small" in lib.gpz_last_error()


def test_reexports_under_the_gpzoo_names():
    import gpzoo.likelihoods as li
    import gpzoo.utilities as ut
    import gpzoo_amd.likelihoods as ali
    import gpzoo_amd.utilities as aut
    for name in ("gene_deviance", "gene_autocorr", "rank_genes", "GeneAutocorr"):
        assert getattr(ut, name) is getattr(aut, name)
    assert ut.GeneAutocorr._fields == ("I", "expected", "variance", "z")
    assert li.SparseCounts.select_genes is ali.SparseCounts.select_genes
    assert li.SparseExpression.select_genes is ali.SparseExpression.select_genes
    import inspect
    sig = inspect.signature(ut.rank_genes)
    assert list(sig.parameters)[:2] == ["counts", "by"] and sig.parameters["by"].default == "deviance"
    assert sig.parameters["coords"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["nfeat"].default is None
    assert inspect.signature(ut.gene_autocorr).parameters["n_neighs"].default == 6
    assert inspect.signature(ut.gene_deviance).parameters["family"].default == "poisson"


def test_moments_from_integer_counts_match_the_dense_weights():
    """``_moran_moments`` runs on any device: here on the CPU against the dense-W oracle."""
    import gene_rank_cases as G
    from gpzoo.utilities import _moran_moments
    for N, K in [g for g in G.GRAPHS if g[0] <= 1037]:
        nbr = G.graph(N, K)
        EI, VI = G.moments_oracle(nbr)
        e, v = _moran_moments(torch.tensor(nbr))
        assert e.dtype == torch.float64 and v.dtype == torch.float64
        assert abs(float(e) - EI) <= 1e-12 * abs(EI) and abs(float(v) - VI) <= G.moments_bound(N, K, VI), (N, K)
