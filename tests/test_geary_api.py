"""The surface of Geary's C and the randomisation moments: the C entries' declarations, bindings, host-only plan queries and
the argument errors that come before any launch (CPU), and ``gene_autocorr(mode=, assumption=)``, ``gene_kurtosis``,
``rank_genes(by="geary")`` and ``dims_autocorr(mode="geary")`` through every path (GPU)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

NEW_SYMBOLS = ("gpz_gene_spatial_stats_sparse", "gpz_gene_spatial_stats_sparse_plan", "gpz_spatial_stats", "gpz_spatial_stats_plan",
               "gpz_gene_autocorr_perm_sparse", "gpz_gene_autocorr_perm_sparse_plan", "gpz_autocorr_perm_rows",
               "gpz_autocorr_perm_rows_plan")
STATS = ["I", "C", "mean", "var", "kurtosis", "info", "partials", "partials_bytes", "stream"]
PERM_OUTPUTS = ["value", "sims", "n_ge", "n_le", "sim_mean", "sim_m2", "info", "partials", "partials_bytes", "stream"]


def header():
    return open(os.path.join(ROOT, "include", "gpzoo_hip.h")).read()


def _args(name):
    args = re.search(rf"\b{name}\s*\(([^;{{]*?)\)\s*;", header(), flags=re.S).group(1)
    return [a.split()[-1].lstrip("*") for a in args.replace("\n", " ").split(",")]


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_new_entries_are_declared_exported_and_bound():
    from gpzoo_amd import _lib, build, ops
    hdr = header()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in hdr and name in _lib.exported_symbols() and hasattr(lib, name)
    assert lib.gpz_version() == 212
    for n in ("gene_spatial_stats_sparse", "spatial_stats", "spatial_stats_plan", "gene_autocorr_perm_sparse", "autocorr_perm_rows",
              "autocorr_perm_plan", "SpatialStats", "AutocorrPerm"):
        assert callable(getattr(ops, n))
    # Geary's closing expression and the wide gene pass are moran_expr.h's; every file that includes it is a source or a
    # header the source hash covers, and every source that does is built with fp contraction off (one kernel, one set of bits)
    assert "spatial_stats.hip" in build.SOURCES and "moran_expr.h" in build.HEADERS
    assert "geary_value" in open(os.path.join(build.CSRC, "moran_expr.h")).read()
    users = [f for f in os.listdir(build.CSRC)
             if f.endswith((".hip", ".h")) and '#include "moran_expr.h"' in open(os.path.join(build.CSRC, f)).read()]
    assert {"spatial_stats.hip", "moran_perm.hip", "gene_rank.hip"} <= set(users) <= set(build.SOURCES + build.HEADERS)
    assert all("-ffp-contract=off" in build.SOURCE_FLAGS[f] for f in users if f.endswith(".hip"))


def test_scratch_is_the_explicit_argument_partials_sized_by_the_plan():
    hdr = header()
    by_gene = ["row_ptr", "row_spot", "row_perm", "col_val"]
    assert _args("gpz_gene_spatial_stats_sparse") == by_gene + ["nbr", "N", "D", "nnz", "K"] + STATS
    assert _args("gpz_spatial_stats") == ["values", "N", "L", "dtype", "nbr", "K"] + STATS
    assert _args("gpz_gene_autocorr_perm_sparse") == by_gene + ["nbr", "perms", "N", "D", "nnz", "K", "P", "stat", "perm_batch",
                                                               "line_mode"] + PERM_OUTPUTS
    assert _args("gpz_autocorr_perm_rows") == ["values", "nbr", "perms", "N", "D", "K", "P", "stat", "perm_batch", "line_mode"] + PERM_OUTPUTS
    plan_outs = ["perm_batch", "line_mode", "workgroups", "partials_bytes"]
    assert _args("gpz_gene_autocorr_perm_sparse_plan") == ["N", "D", "nnz", "K", "P", "stat", "perm_batch_wanted", "line_mode_wanted"] + plan_outs
    assert _args("gpz_autocorr_perm_rows_plan") == ["N", "D", "K", "P", "stat", "perm_batch_wanted", "line_mode_wanted"] + plan_outs
    assert _args("gpz_gene_spatial_stats_sparse_plan") == ["N", "D", "nnz", "K", "gene_chunk", "workgroups", "partials_bytes"]
    assert _args("gpz_spatial_stats_plan") == ["N", "L", "K", "row_chunk", "chunks", "partials_bytes"]
    for name in NEW_SYMBOLS:
        assert "ws" not in _args(name) and f"{name}_workspace_bytes" not in hdr
        if not name.endswith("_plan"):
            assert _args(name)[-3:] == ["partials", "partials_bytes", "stream"]
    import scratch_cases as S
    assert not set(NEW_SYMBOLS) & S.header_entries_with_workspace(hdr)


def test_plan_queries_need_no_device():
    from gpzoo_amd import ops
    N, D, K, P = 39694, 17702, 6, 100
    sp = ops.spatial_stats_plan(N, K, D=D, nnz=35_000_000)
    assert sp == ops.gene_rank_plan(N, D, 35_000_000, K=K)                    # the Moran entry's line handling and scratch
    assert sp["partials_bytes"] >= sp["workgroups"] * N * 4 + N * 4 and sp["gene_chunk"] == 256
    cols = ops.spatial_stats_plan(N, K, L=65)
    assert cols["row_chunk"] == 256 and cols["chunks"] == -(-N // 256)
    assert cols["chunks"] * 65 * 40 + 65 * 8 <= cols["partials_bytes"] <= cols["chunks"] * 65 * 40 + 65 * 8 + 512
    for stat in ("moran", "geary"):                                           # the statistic does not change the plan
        assert ops.autocorr_perm_plan(N, D, K, P, nnz=1000, stat=stat) == ops.morans_perm_plan(N, D, K, P, nnz=1000)
        assert ops.autocorr_perm_plan(N, D, K, P, stat=stat, perm_batch=3, line_mode="global") == ops.morans_perm_plan(
            N, D, K, P, perm_batch=3, line_mode="global")
    for bad in ("Moran", 1, None, "c"):
        with pytest.raises(ValueError, match="stat"):
            ops.autocorr_perm_plan(N, D, K, P, stat=bad)
    for bad in (dict(K=0), dict(K=33), dict(N=6), dict(D=0)):
        with pytest.raises(ValueError):
            ops.spatial_stats_plan(**{**dict(N=N, K=K, D=D, nnz=5), **bad})
    for bad in (dict(K=0), dict(N=6), dict(L=0), dict(L=(1 << 20) + 1)):
        with pytest.raises(ValueError):
            ops.spatial_stats_plan(**{**dict(N=N, K=K, L=4), **bad})
    with pytest.raises(ValueError, match="does not fit"):
        ops.autocorr_perm_plan(50000, D, K, P, stat="geary", line_mode="lds")


def test_bad_arguments_are_refused_before_any_launch_with_the_entrys_name():
    from gpzoo_amd import _lib
    lib = _lib.load()
    # host memory stands in for device memory: every refusal below comes before the first launch
    buf = (C.c_char * 16384)()
    base = (C.addressof(buf) + 15) & ~15
    p = lambda off=0: C.c_void_p(base + off)  # noqa: E731
    ins = [p(256 * i) for i in range(6)]
    outs = [p(2048 + 256 * i) for i in range(7)]

    def err():
        return lib.gpz_last_error()

    def sparse(ins=ins, N=10, D=4, nnz=5, K=6, P=3, stat=1, pb=0, mode=0, outs=outs, scratch=p(8192), nbytes=1 << 30):
        return lib.gpz_gene_autocorr_perm_sparse(*ins, N, D, nnz, K, P, stat, pb, mode, *outs, scratch, nbytes, None)

    def rows(ins=ins[:3], N=10, D=4, K=6, P=3, stat=1, pb=0, mode=0, outs=outs, scratch=p(8192), nbytes=1 << 30):
        return lib.gpz_autocorr_perm_rows(*ins, N, D, K, P, stat, pb, mode, *outs, scratch, nbytes, None)
    for f, who in ((sparse, b"gpz_gene_autocorr_perm_sparse"), (rows, b"gpz_autocorr_perm_rows")):
        assert f(ins=[None] + ins[1:6 if f is sparse else 3]) < 0 and who + b": null pointer" in err()
        for i in (0, 2, 3, 4, 5, 6):                                  # every output but sims is needed
            assert f(outs=outs[:i] + [None] + outs[i + 1:]) < 0 and who + b": null pointer" in err()
        assert f(scratch=None) < 0 and who + b": null pointer" in err()
        assert f(N=0) < 0 and who + b": bad extents" in err()
        assert f(D=1 << 31) < 0 and who in err() and b"32 bits" in err()
        for stat in (-1, 2):
            assert f(stat=stat) < 0 and who + b": stat" in err() and b"unknown" in err()
        for stat in (0, 1):
            for K in (0, 33, 10):
                assert f(stat=stat, K=K) < 0 and who + b": K" in err() and b"neighbours of N = 10 spots unsupported" in err()
            assert f(stat=stat, P=0) < 0 and who + b": P = 0 permutations" in err()
            assert f(stat=stat, pb=33) < 0 and who + b": perm_batch = 33" in err()
            assert f(stat=stat, mode=3) < 0 and who + b": line_mode 3 unknown" in err()
            assert f(stat=stat, N=50000, K=6, mode=2) < 0 and who in err() and b"does not fit" in err()
            assert f(stat=stat, scratch=p(8200)) < 0 and who in err() and b"16-byte aligned" in err()
            assert f(stat=stat, nbytes=64) < 0 and who + b": partials too small" in err()
    assert sparse(ins=ins[:2] + [None] + ins[3:]) < 0 and b"gpz_gene_autocorr_perm_sparse: null pointer (non-zeros)" in err()

    def stats(ins=ins[:5], N=10, D=4, nnz=5, K=6, outs=outs[:6], scratch=p(8192), nbytes=1 << 30):
        return lib.gpz_gene_spatial_stats_sparse(*ins, N, D, nnz, K, *outs, scratch, nbytes, None)

    def cols(values=p(0), N=10, L=4, dtype=0, nbr=p(256), K=6, outs=outs[:6], scratch=p(8192), nbytes=1 << 30):
        return lib.gpz_spatial_stats(values, N, L, dtype, nbr, K, *outs, scratch, nbytes, None)
    who = b"gpz_gene_spatial_stats_sparse"
    assert stats(ins=[None] + ins[1:5]) < 0 and who + b": null pointer" in err()
    assert stats(ins=ins[:4] + [None]) < 0 and who + b": null pointer" in err()
    assert stats(outs=outs[:5] + [None]) < 0 and who + b": null pointer" in err()            # info
    assert stats(scratch=None) < 0 and who + b": null pointer" in err()
    assert stats(ins=ins[:1] + [None] + ins[2:5]) < 0 and who + b": null pointer (non-zeros)" in err()
    assert stats(N=0) < 0 and who + b": bad extents" in err()
    assert stats(nnz=1 << 31) < 0 and who in err() and b"32 bits" in err()
    for K in (0, 33, 10):
        assert stats(K=K) < 0 and who + b": K" in err()
    assert stats(scratch=p(8200)) < 0 and who + b": partials must be 16-byte aligned" in err()
    assert stats(nbytes=64) < 0 and who + b": partials too small" in err()
    who = b"gpz_spatial_stats"
    assert cols(values=None) < 0 and who + b": null pointer" in err()
    assert cols(nbr=None) < 0 and who + b": null pointer" in err()
    assert cols(outs=outs[:5] + [None]) < 0 and who + b": null pointer" in err()
    assert cols(scratch=None) < 0 and who + b": null pointer" in err()
    assert cols(dtype=2) < 0 and who + b": unknown dtype 2" in err()
    for K in (0, 10):
        assert cols(K=K) < 0 and who + b": N=10" in err()
    assert cols(L=0) < 0 and who + b": L=0" in err()
    assert cols(scratch=p(8200)) < 0 and who + b": partials must be 16-byte aligned" in err()
    assert cols(nbytes=64) < 0 and who + b": partials too small" in err()


def test_the_python_surface():
    import gpzoo.utilities as U
    import gpzoo_amd.utilities as A
    for name in ("GeneGeary", "GeneGearyPerm", "gene_kurtosis", "gene_autocorr", "rank_genes", "dims_autocorr"):
        assert getattr(U, name) is getattr(A, name)
    assert A.GeneGeary._fields == ("C", "expected", "variance", "z")
    assert A.GeneGearyPerm._fields == ("C",) + A.GeneAutocorrPerm._fields[1:]
    sig = inspect.signature(A.gene_autocorr)
    assert [sig.parameters[k].default for k in ("mode", "assumption")] == ["moran", "normality"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("mode", "assumption"))
    assert inspect.signature(A.dims_autocorr).parameters["mode"].default == "moran"
    doc = " ".join(A.gene_autocorr.__doc__.split())
    assert "negative for positive autocorrelation" in doc and "VC_rand" in doc and "N >= 4" in doc
    assert "NEGATIVE z" in " ".join(A.GeneGeary.__doc__.split()) and "pval_less" in A.GeneGearyPerm.__doc__


def test_argument_errors_come_before_any_device_work():
    from gpzoo.likelihoods import SparseCounts
    from gpzoo.utilities import dims_autocorr, gene_autocorr, gene_kurtosis, rank_genes
    from gpzoo_amd import ops
    V = torch.rand(5, 9)
    c = SparseCounts(torch.tensor(np.random.default_rng(0).poisson(0.7, size=(5, 9)).astype(np.float32)))
    nbr = torch.stack([(torch.arange(9) + s) % 9 for s in (1, 2)], dim=1)
    perms = torch.stack([torch.randperm(9) for _ in range(3)]).to(torch.int32)
    for bad in ("Geary", "c", None, 1):
        with pytest.raises(ValueError, match="mode"):
            gene_autocorr(V, graph=nbr, mode=bad)
        with pytest.raises(ValueError, match="mode"):
            dims_autocorr(V.T, torch.rand(9, 2), mode=bad)
    for bad in ("normal", "randomization", None):
        with pytest.raises(ValueError, match="assumption"):
            gene_autocorr(V, graph=nbr, assumption=bad)
    for mode in ("moran", "geary"):
        with pytest.raises(ValueError, match="N >= 4"):
            gene_autocorr(torch.rand(5, 3), graph=torch.tensor([[1], [2], [0]]), mode=mode, assumption="randomisation")
    with pytest.raises(ValueError, match="by='geary' needs coords"):
        rank_genes(c, by="geary")
    with pytest.raises(ValueError, match="'geary'"):
        rank_genes(c, by="gearys_c")
    with pytest.raises(ValueError):
        gene_kurtosis(torch.rand(9))
    with pytest.raises(RuntimeError, match="GPU only"):
        gene_kurtosis(c)
    for call in (lambda: ops.gene_spatial_stats_sparse(c, nbr), lambda: ops.spatial_stats(V.T.contiguous(), nbr),
                 lambda: ops.gene_autocorr_perm_sparse(c, nbr, perms, stat="geary"), lambda: ops.autocorr_perm_rows(V, nbr, perms, stat="geary")):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    with pytest.raises(TypeError, match="view"):
        ops.gene_spatial_stats_sparse(c[:, torch.arange(4)], nbr)
    with pytest.raises(TypeError):
        ops.gene_autocorr_perm_sparse(V, nbr, perms, stat="geary")
    with pytest.raises(ValueError, match="float32"):
        ops.autocorr_perm_rows(V.double(), nbr, perms, stat="geary")
    for bad in ("Geary", 1, None):
        with pytest.raises(ValueError, match="stat"):
            ops.gene_autocorr_perm_sparse(c, nbr, perms, stat=bad)
        with pytest.raises(ValueError, match="stat"):
            ops.autocorr_perm_rows(V, nbr, perms, stat=bad)


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def _i64(t):
    return t.cpu().numpy().view(np.int64)


def _case(N=1037, K=6):
    import gene_rank_cases as G
    import moran_perm_cases as M
    from gpzoo.likelihoods import SparseCounts
    c = SparseCounts(torch.tensor(M.dense(N, "counts"))).cuda()
    return c, torch.tensor(M.dense(N, "counts")).cuda(), torch.tensor(G.graph(N, K)).cuda(), torch.tensor(M.perms(N)).cuda()


@pytest.mark.gpu
def test_the_defaults_are_todays_call_bit_for_bit():
    from gpzoo.utilities import GeneAutocorr, GeneAutocorrPerm, gene_autocorr
    c, dense, nbr, perms = _case()
    for values in (c, dense):
        a, b = gene_autocorr(values, graph=nbr), gene_autocorr(values, graph=nbr, mode="moran", assumption="normality")
        assert type(a) is type(b) is GeneAutocorr
        for f in GeneAutocorr._fields:
            np.testing.assert_array_equal(_i64(getattr(a, f)), _i64(getattr(b, f)), err_msg=f)
        a = gene_autocorr(values, graph=nbr, perms=perms, return_sims=True)
        b = gene_autocorr(values, graph=nbr, perms=perms, return_sims=True, mode="moran", assumption="normality")
        assert type(a) is type(b) is GeneAutocorrPerm and a.variance.dim() == 0
        for f in GeneAutocorrPerm._fields:
            x, y = getattr(a, f), getattr(b, f)
            assert x == y if f == "n_perms" else torch.equal(torch.nan_to_num(x.double(), nan=-7.0), torch.nan_to_num(y.double(), nan=-7.0)), f


@pytest.mark.gpu
def test_gene_autocorr_geary_and_randomisation_through_every_path():
    import gene_rank_cases as G
    import geary_cases as Y
    import moran_perm_cases as M
    from gpzoo.utilities import GeneAutocorr, GeneAutocorrPerm, GeneGeary, GeneGearyPerm, gene_autocorr, gene_kurtosis
    from gpzoo_amd import ops
    N, K = 1037, 6
    c, dense, nbr, perms = _case(N, K)
    nan = np.isnan(Y.observed_oracle(N, K, "counts"))
    s = ops.gene_spatial_stats_sparse(c, nbr)
    g = gene_autocorr(c, graph=nbr, mode="geary")
    assert type(g) is GeneGeary and float(g.expected) == 1.0 and g.variance.dim() == 0
    np.testing.assert_array_equal(_i64(g.C), _i64(s.C))
    want = Y.moments(G.graph(N, K), s.kurtosis.cpu().numpy())
    assert abs(float(g.variance) - want["VC_norm"]) <= Y.moments_bound(N, K, want["VC_norm"])
    np.testing.assert_allclose(g.z.cpu().numpy()[~nan], ((s.C - 1.0) / want["VC_norm"] ** 0.5).cpu().numpy()[~nan], rtol=1e-11)
    for mode, kind, value, key in (("moran", GeneAutocorr, s.I, "VI_rand"), ("geary", GeneGeary, s.C, "VC_rand")):
        r = gene_autocorr(c, graph=nbr, mode=mode, assumption="randomisation")
        assert type(r) is kind and r.variance.shape == (G.D,) and r.z.shape == (G.D,)
        np.testing.assert_array_equal(_i64(r[0]), _i64(value))
        got = r.variance.cpu().numpy()
        np.testing.assert_array_equal(np.isnan(got), nan)
        assert (np.abs(got - want[key])[~nan] <= Y.moments_bound(N, K, want[key])[~nan]).all()
        assert (got[~nan] > 0).all()
        np.testing.assert_allclose(r.z.cpu().numpy()[~nan], ((value - r.expected) / r.variance.sqrt()).cpu().numpy()[~nan], rtol=1e-15)
    # permutations: the counts of the permutation entry, the observed C of the stats entry, pval_less towards small C
    p = gene_autocorr(c, graph=nbr, perms=perms, mode="geary", return_sims=True)
    q = ops.gene_autocorr_perm_sparse(c, nbr, perms, stat="geary", return_sims=True)
    assert type(p) is GeneGearyPerm and p.n_perms == M.P and torch.equal(p.n_ge, q.n_ge) and torch.equal(p.n_le, q.n_le)
    np.testing.assert_array_equal(_i64(p.C), _i64(s.C))
    n_ge, n_le = Y.counts_oracle_exact(N, K)
    ulps = dict(rtol=4 * np.finfo(np.float64).eps, atol=0)
    np.testing.assert_allclose(p.pval_less.cpu().numpy()[~nan], (n_le[~nan] + 1) / (M.P + 1), **ulps)
    np.testing.assert_allclose(p.pval_greater.cpu().numpy()[~nan], (n_ge[~nan] + 1) / (M.P + 1), **ulps)
    for f in ("pval_greater", "pval_less", "pval_sim", "mean_sim", "var_sim", "z_sim", "pval_z_sim"):
        assert np.isnan(getattr(p, f).cpu().numpy()[nan]).all(), f
    seeded = [gene_autocorr(c, graph=nbr, n_perms=7, seed=3, mode="geary", assumption="randomisation") for _ in range(2)]
    assert seeded[0].n_perms == 7 and seeded[0].variance.shape == (G.D,) and torch.equal(seeded[0].n_le, seeded[1].n_le)
    # a dense tensor: the columns entry for C and b2, the rows entry for the counts
    d = gene_autocorr(dense, graph=nbr, perms=perms, mode="geary", assumption="randomisation")
    cols = ops.spatial_stats(dense.T.contiguous(), nbr)
    assert type(d) is GeneGearyPerm and torch.equal(d.n_ge, p.n_ge) and torch.equal(d.n_le, p.n_le)
    np.testing.assert_array_equal(_i64(d.C), _i64(cols.C))
    want_d = Y.moments(G.graph(N, K), cols.kurtosis.cpu().numpy())["VC_rand"]
    assert (np.abs(d.variance.cpu().numpy() - want_d)[~nan] <= Y.moments_bound(N, K, want_d)[~nan]).all()
    # gene_kurtosis: the stats entries' b2, whatever graph they are given
    for values, b2 in ((c, s.kurtosis), (dense, cols.kurtosis)):
        k = gene_kurtosis(values)
        assert k.shape == (G.D,) and k.dtype == torch.float64 and k.is_cuda
        np.testing.assert_allclose(k.cpu().numpy(), b2.cpu().numpy(), rtol=Y.KURTOSIS_RTOL, equal_nan=True)
    np.testing.assert_allclose(gene_kurtosis(c).cpu().numpy(), Y.kurtosis_oracle(M.dense(N, "counts"))["kurtosis"], rtol=Y.KURTOSIS_RTOL,
                               equal_nan=True)


@pytest.mark.gpu
def test_rank_genes_by_geary_and_dims_autocorr_geary():
    import gene_rank_cases as G
    import geary_cases as Y
    from gpzoo.likelihoods import SparseCounts
    from gpzoo.utilities import dims_autocorr, gene_autocorr, log_normalize, rank_genes
    from gpzoo_amd import ops
    N, K = 1037, 6
    c = SparseCounts(torch.tensor(G.counts(N, "full"))).cuda()
    nbr = torch.tensor(G.graph(N, K)).cuda()
    order, score = rank_genes(c, by="geary", graph=nbr)
    C = gene_autocorr(log_normalize(c, center=False), graph=nbr, mode="geary").C
    same = lambda a, b: torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))  # noqa: E731
    assert order.shape == (G.D,) and same(score, (1.0 - C)[order])
    nan = torch.isnan(score)
    n_nan = int(nan.sum())
    assert n_nan >= 1 and bool(nan[G.D - n_nan:].all()) and not bool(nan[:G.D - n_nan].any())          # NaN last
    assert bool((score[:G.D - n_nan][1:] <= score[:G.D - n_nan][:-1]).all())                           # decreasing 1 - C
    top, _ = rank_genes(c, by="geary", graph=nbr, nfeat=5)
    assert torch.equal(top, order[:5])
    coords = torch.tensor(np.random.default_rng(3).uniform(size=(N, 2))).cuda()
    o2, s2 = rank_genes(c, by="geary", coords=coords)
    assert same(s2, (1.0 - gene_autocorr(log_normalize(c, center=False), coords, mode="geary").C)[o2])
    # dims_autocorr: increasing C, NaN last; the default unchanged
    F = np.random.default_rng(4).normal(size=(N, 5))
    F[:, 2] = 1.5
    F[:, 4] = np.linspace(0, 1, N) + coords.cpu().numpy()[:, 0]
    idx, Cs = dims_autocorr(F, coords.cpu().numpy(), mode="geary")
    graph = ops.spatial_knn(coords, 6)
    want = Y.geary_oracle(F.T, graph.cpu().numpy())
    assert idx.dtype == np.int64 and idx[-1] == 2 and np.isnan(Cs[-1]) and (np.diff(Cs[:-1]) >= 0).all()
    np.testing.assert_allclose(Cs, want[idx], rtol=0, atol=Y.GEARY_ATOL_ROWS, equal_nan=True)
    i0, I0 = dims_autocorr(F, coords.cpu().numpy())
    np.testing.assert_array_equal(I0.view(np.int64), ops.morans_i(torch.tensor(F).cuda(), graph).cpu().numpy()[i0].view(np.int64))
