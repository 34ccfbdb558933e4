"""CPU: the surface of the residual entries -- the C entries' declarations, bindings and host-side refusals, the plan query
and its 256 MiB rule, the refusals of the ops and model entries before any device work, and the re-exports under the
``gpzoo`` names."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

NEW_SYMBOLS = ("gpz_count_residuals", "gpz_count_residuals_sparse", "gpz_residual_morans_i", "gpz_residual_morans_i_sparse",
               "gpz_residual_morans_i_plan")


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
    assert all(n in comment for n in NEW_SYMBOLS)
    assert all(callable(getattr(ops, n)) for n in ("count_residuals", "residual_morans_i", "residual_autocorr_plan"))
    assert "residual.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "residual.hip"))
    # the Moran pass is spatial_stats.hip's, reached through one internal header the source hash covers; it is built with
    # fp contraction off, and so is spatial.hip still (the kNN distances)
    assert "moran_pass.h" in build.HEADERS and "spatial_stats.hip" in build.SOURCES
    assert build.SOURCE_FLAGS["spatial_stats.hip"] == ["-ffp-contract=off"] and build.SOURCE_FLAGS["spatial.hip"] == ["-ffp-contract=off"]
    text = open(os.path.join(build.CSRC, "residual.hip")).read()
    assert '#include "moran_pass.h"' in text and '#include "gene_rows.h"' in text and "void mi_rows" not in text
    home = open(os.path.join(build.CSRC, "spatial_stats.hip")).read()
    assert '#include "moran_pass.h"' in home and "void mi_rows" in home
    assert "void mi_rows" not in open(os.path.join(build.CSRC, "spatial.hip")).read()
    # the argument counts of the bindings are the header's
    for name in NEW_SYMBOLS:
        assert len(_lib._SIGNATURES[name][1]) == len(_args(name)), name


def test_scratch_is_the_explicit_argument_partials_sized_by_the_plan():
    hdr = header()
    for name in NEW_SYMBOLS[:4]:
        a = _args(name)
        assert a[-3:] == ["partials", "partials_bytes", "stream"] and "ws" not in a and "ws_bytes" not in a
        assert f"{name}_workspace_bytes" not in hdr
    assert _args("gpz_residual_morans_i_plan") == ["B", "D", "Lt", "nnz", "slab_genes_wanted", "slab_genes", "n_slabs",
                                                   "spots_per_tile", "genes_per_block", "spot_slices", "gene_chunk",
                                                   "factors_padded", "partials_bytes"]
    assert _args("gpz_residual_morans_i")[:8] == ["mean", "scale", "W", "V", "theta", "y", "genes", "nbr"]
    assert _args("gpz_residual_morans_i")[-8:-3] == ["slab_genes", "I", "res_mean", "res_var", "info"]
    import scratch_cases as S
    assert not set(NEW_SYMBOLS) & S.header_entries_with_workspace(hdr)


def test_no_existing_entry_gained_a_workspace():
    """The header's entries with a ``ws`` argument or a ``_workspace_bytes`` companion are the closed table of
    tests/scratch_cases.py, as before."""
    import scratch_cases as S
    hdr = header()
    with_ws = S.header_entries_with_workspace(hdr)
    assert with_ws and with_ws <= {e for r in S.ROWS for e in r.entries}
    companions = set(re.findall(r"\b(gpz_\w+)_workspace_bytes\s*\(", hdr))
    assert not any("residual" in n for n in companions | with_ws)
    assert _args("gpz_morans_i")[-3:] == ["ws", "ws_bytes", "stream"] and len(_args("gpz_morans_i")) == 11


def test_plan_query_needs_no_device_and_obeys_the_256_mib_rule():
    from gpzoo_amd import ops
    p = ops.residual_autocorr_plan(39694, 17702, 20)
    assert set(p) == {"slab_genes", "n_slabs", "spots_per_tile", "genes_per_block", "spot_slices", "gene_chunk", "factors_padded",
                      "partials_bytes"}
    assert (p["spots_per_tile"], p["genes_per_block"], p["gene_chunk"], p["factors_padded"]) == (64, 64, 512, 20)
    for B, D in ((39694, 17702), (7000, 17702), (4099, 3000), (600, 130), (7, 1), (100000, 64), (2_000_000, 500)):
        p = ops.residual_autocorr_plan(B, D, 20)
        sg, cap, d64 = p["slab_genes"], (256 << 20) // (4 * B), -(-D // 64) * 64
        assert sg % 64 == 0 and 64 <= sg <= d64
        assert sg == max(64, min(cap // 64 * 64, d64, 1 << 20))               # the largest multiple of 64 within 256 MiB
        assert p["n_slabs"] == -(-D // sg) and 1 <= p["spot_slices"] <= 16
        # the scratch: the slab, plus O(B Lt) factors, O(B / 256 x slab) partial sums and the slab's means --
        # nothing of D x B or nnz elements
        assert 4 * B * sg <= p["partials_bytes"] <= 4 * B * sg + 4 * 21 * (B + 64) + (24 * (B // 256 + 1) + 8) * sg + 8192
        assert ops.residual_autocorr_plan(B, D, 20, nnz=10 ** 9)["partials_bytes"] == p["partials_bytes"]
    # the override: a positive multiple of 64, cut to D rounded up to 64
    assert ops.residual_autocorr_plan(600, 130, 5, 0, 64)["n_slabs"] == 3
    assert ops.residual_autocorr_plan(600, 130, 5, 0, 128)["slab_genes"] == 128
    assert ops.residual_autocorr_plan(600, 130, 5, 0, 192) == ops.residual_autocorr_plan(600, 130, 5, 0, 6400)
    assert ops.residual_autocorr_plan(600, 130, 5)["slab_genes"] == 192
    for bad in ((0, 1, 1, 0, 0), (5, 0, 1, 0, 0), (5, 1, 0, 0, 0), (5, 1, 65, 0, 0), (1 << 31, 1, 1, 0, 0), (5, 1 << 31, 1, 0, 0),
                (5, 1, 1, 1 << 31, 0), (5, 1, 1, -1, 0), (5, 1, 1, 0, 32), (5, 1, 1, 0, 100), (5, 1, 1, 0, -64)):
        with pytest.raises(ValueError):
            ops.residual_autocorr_plan(*bad)


def test_bad_arguments_are_refused_before_any_launch():
    from gpzoo_amd import _lib
    lib = _lib.load()
    # host memory stands in for device memory: every refusal below comes before the first launch
    buf = (C.c_char * 16384)()
    base = (C.addressof(buf) + 15) & ~15
    p = lambda off=0: C.c_void_p(base + off)  # noqa: E731
    inp = [p(256 * i) for i in range(8)]            # mean, scale, W, V, theta, y, genes, nbr
    outs = [p(4096 + 256 * i) for i in range(4)]    # I, res_mean, res_var, info

    def run(inp=inp, B=10, D=4, G=4, Lt=3, K=2, family=1, kind=0, slab=0, outs=outs, scratch=p(8192), nbytes=1 << 30):
        return lib.gpz_residual_morans_i(*inp, B, D, G, Lt, K, family, kind, 1, slab, *outs, scratch, nbytes, None)
    who = b"gpz_residual_morans_i: "
    for i in (0, 1, 2, 3, 5, 7):
        assert run(inp=inp[:i] + [None] + inp[i + 1:]) < 0 and who + b"null pointer" in lib.gpz_last_error(), i
    assert run(inp=inp[:4] + [None] + inp[5:]) < 0 and b"needs theta" in lib.gpz_last_error()
    assert run(inp=inp[:4] + [None] + inp[5:], family=0, nbytes=8) < 0 and b"partials too small" in lib.gpz_last_error()
    for i in range(4):
        assert run(outs=outs[:i] + [None] + outs[i + 1:]) < 0 and who + b"null pointer" in lib.gpz_last_error()
    assert run(scratch=None) < 0 and who + b"null pointer" in lib.gpz_last_error()
    for K in (0, -1, 33, 10):
        assert run(K=K) < 0 and b"neighbours" in lib.gpz_last_error(), K
    assert run(B=3, K=3) < 0 and b"neighbours" in lib.gpz_last_error()
    for Lt in (0, 65):
        assert run(Lt=Lt) < 0 and b"factors unsupported" in lib.gpz_last_error()
    for slab in (1, 63, 100, -64):
        assert run(slab=slab) < 0 and b"multiple of 64" in lib.gpz_last_error()
    assert run(family=2) < 0 and b"family 2 unknown" in lib.gpz_last_error()
    assert run(kind=2) < 0 and b"kind 2 unknown" in lib.gpz_last_error()
    assert run(B=0) < 0 and b"bad extents" in lib.gpz_last_error()
    assert run(B=1 << 31) < 0 and b"32 bits" in lib.gpz_last_error()
    assert run(D=1 << 31) < 0 and b"32 bits" in lib.gpz_last_error()
    assert run(inp=inp[:6] + [None] + inp[7:], G=3) < 0 and b"without a list" in lib.gpz_last_error()
    assert run(scratch=p(8196)) < 0 and b"16-byte aligned" in lib.gpz_last_error()
    assert run(nbytes=8) < 0 and b"partials too small" in lib.gpz_last_error()
    # the sparse entry: the by-gene arrays, nnz
    rows = [p(12288 + 256 * i) for i in range(4)]

    def sparse(rows=rows, nnz=5, B=10):
        return lib.gpz_residual_morans_i_sparse(*inp[:5], *rows, inp[6], inp[7], B, 4, nnz, 4, 3, 2, 1, 0, 1, 0, *outs, p(8192), 1 << 30, None)
    assert sparse(rows=[None] + rows[1:]) < 0 and b"null pointer (counts)" in lib.gpz_last_error()
    assert sparse(rows=[rows[0], None] + rows[2:]) < 0 and b"null pointer (non-zeros)" in lib.gpz_last_error()
    assert sparse(nnz=1 << 31) < 0 and b"32 bits" in lib.gpz_last_error()
    assert sparse(nnz=-1) < 0 and b"bad extents" in lib.gpz_last_error()
    # the residual entries
    out = p(4096)
    assert lib.gpz_count_residuals(*inp[:7], 10, 4, 4, 3, 1, 0, 1, None, p(8192), 1 << 30, None) < 0
    assert b"gpz_count_residuals: null pointer" in lib.gpz_last_error()
    assert lib.gpz_count_residuals(*inp[:7], 10, 4, 4, 3, 1, 3, 1, out, p(8192), 1 << 30, None) < 0 and b"kind 3" in lib.gpz_last_error()
    assert lib.gpz_count_residuals(*inp[:7], 10, 4, 4, 3, 1, 0, 1, out, p(8192), 8, None) < 0 and b"partials too small" in lib.gpz_last_error()
    assert lib.gpz_count_residuals_sparse(*inp[:5], None, *rows[1:], inp[6], 10, 4, 5, 4, 3, 1, 0, 1, out, p(8192), 1 << 30, None) < 0
    assert b"gpz_count_residuals_sparse: null pointer (counts)" in lib.gpz_last_error()


def _case(D=9, B=13, Lt=2):
    g = torch.Generator().manual_seed(0)
    return dict(mean=torch.randn(Lt, B, generator=g), scale=torch.rand(Lt, B, generator=g), W=torch.rand(D, Lt, generator=g),
                V=torch.ones(B), y=torch.poisson(torch.rand(D, B, generator=g)), theta=torch.ones(D))


def test_ops_refusals_come_before_any_device_work():
    from gpzoo import utilities as ut
    from gpzoo.likelihoods import SparseCounts
    from gpzoo_amd import ops
    c = _case()
    a = (c["mean"], c["scale"], c["W"], c["V"])
    nbr = torch.stack([(torch.arange(13) + k + 1) % 13 for k in range(3)], dim=1)
    sc = SparseCounts(c["y"])
    view = sc[:, torch.tensor([0, 2, 5])]
    for bad, match in ((view, "a view"), (sc.T, "obs x feat"), (ut.log_normalize(sc), "not counts"), (np.zeros((9, 13)), "dense")):
        with pytest.raises(TypeError, match=match):
            ops.count_residuals(*a, bad)
        with pytest.raises(TypeError, match=match):
            ops.residual_morans_i(*a, bad, nbr)
    for kind in ("anscombe", 0, None):
        with pytest.raises(ValueError, match="kind"):
            ops.count_residuals(*a, c["y"], kind=kind)
        with pytest.raises(ValueError, match="kind"):
            ops.residual_morans_i(*a, sc, nbr, kind=kind)
    # shapes
    with pytest.raises(ValueError, match="do not fit together"):
        ops.count_residuals(c["mean"], c["scale"][:, :5], c["W"], c["V"], c["y"])
    with pytest.raises(ValueError, match="do not fit together"):
        ops.count_residuals(c["mean"], c["scale"], c["W"][:4], c["V"], c["y"])
    with pytest.raises(ValueError, match="do not fit together"):
        ops.count_residuals(*a, c["y"][:, :12])
    with pytest.raises(ValueError, match="do not fit together"):
        ops.count_residuals(*a, sc, theta_pos=torch.ones(8))
    with pytest.raises(ValueError, match="nbr"):
        ops.residual_morans_i(*a, c["y"], nbr[:12])
    with pytest.raises(ValueError, match="nbr"):
        ops.residual_morans_i(*a, c["y"], nbr.float())
    # K outside 1..32, K >= B
    with pytest.raises(ValueError, match="neighbours"):
        ops.residual_morans_i(*a, c["y"], nbr[:, :0])
    with pytest.raises(ValueError, match="neighbours"):
        ops.residual_morans_i(*a, c["y"], torch.zeros(13, 33, dtype=torch.int64))
    with pytest.raises(ValueError, match="neighbours"):
        ops.residual_morans_i(*a, c["y"], torch.zeros(13, 13, dtype=torch.int64))
    for slab in (1, 63, 100, -64, 64.5):
        with pytest.raises(ValueError, match="slab_genes"):
            ops.residual_morans_i(*a, c["y"], nbr, slab_genes=slab)
    # gene lists
    for genes, exc in (([9], IndexError), ([-1, 0], IndexError), ([], ValueError), ([[0, 1]], ValueError), ([0.5], ValueError)):
        with pytest.raises(exc, match="gene"):
            ops.count_residuals(*a, c["y"], genes=genes)
    # whole CPU inputs pass every check and stop at the device
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.count_residuals(*a, c["y"], theta_pos=c["theta"], genes=[3, 3, 0])
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.residual_morans_i(*a, sc, nbr, kind="deviance", slab_genes=64)


def _nsf(likelihood="poisson"):
    import gpzoo.gp as G
    import gpzoo.kernels as K
    from gpzoo.likelihoods import NSF
    c = _case()
    gp = G.WSVGP(K.NSF_RBF(L=2, lengthscale=2.0), dim=2, M=4, jitter=1e-2)
    return NSF(gp, c["y"], L=2, likelihood=likelihood), torch.rand(13, 2), c["y"]


def test_model_refusals_need_no_device():
    model, X, y = _nsf()
    for method, extra in ((model.residual_autocorr, ()), (model.residuals, ([0, 1],))):
        with pytest.raises(ValueError, match="kind"):
            method(X, y, *extra, kind="raw")
        with pytest.raises(ValueError, match="family"):
            method(X, y, *extra, family="gaussian")
        with pytest.raises(ValueError, match='theta= belongs to family="nb"'):
            method(X, y, *extra, family="poisson", theta=3.0)
        with pytest.raises(ValueError, match='theta= belongs to family="nb"'):          # family="model" on a Poisson fit
            method(X, y, *extra, theta=3.0)
        with pytest.raises(ValueError, match="needs theta="):
            method(X, y, *extra, family="nb")
        with pytest.raises(ValueError, match="theta has 3 values"):
            method(X, y, *extra, family="nb", theta=[1.0, 2.0, 3.0])


def test_methods_and_reexports():
    import gpzoo.likelihoods as li
    import gpzoo_amd.likelihoods as ali
    for name in ("residual_autocorr", "count_residuals", "ResidualAutocorr"):
        assert getattr(li, name) is getattr(ali, name)
    assert li.ResidualAutocorr._fields == ("I", "expected", "variance", "z", "residual_mean", "residual_var")
    sig = inspect.signature(li.residual_autocorr)
    assert list(sig.parameters)[:5] == ["qF_list", "W_list", "V_pos", "y", "nbr"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("theta_pos", "kind", "lognormal_mean"))
    assert sig.parameters["kind"].default == "pearson" and sig.parameters["theta_pos"].default is None
    assert list(inspect.signature(li.count_residuals).parameters)[:5] == ["qF_list", "W_list", "V_pos", "y", "genes"]
    doc = " ".join(li.residual_autocorr.__doc__.split())
    assert "normal approximation" in doc and "degrees of freedom" in doc and "not a calibrated test" in doc
    for cls in (li.NSF2, li.NSF, li.MGGP_NSF, li.Hybrid_NSF2, li.Hybrid_NSF_Exact, li.Hybrid_NSF):
        s = inspect.signature(cls.residual_autocorr)
        assert list(s.parameters)[:5] == ["self", "X", "y", "idx", "V"]
        for k, default in (("kind", "pearson"), ("family", "model"), ("theta", None), ("n_neighs", 6), ("graph", None),
                           ("lognormal_mean", True)):
            assert s.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and s.parameters[k].default == default
        assert list(inspect.signature(cls.residuals).parameters)[:6] == ["self", "X", "y", "genes", "idx", "V"]
        assert inspect.signature(cls.deviance).parameters["family"].default == "poisson"       # unchanged
        assert "standardised by the model's own variance" in " ".join(cls.residual_autocorr.__doc__.split())
    assert not hasattr(li.PNMF, "residual_autocorr") and not hasattr(li.RSF, "residual_autocorr")
    ops_sig = inspect.signature(__import__("gpzoo_amd.ops", fromlist=["x"]).count_residuals)
    assert list(ops_sig.parameters) == ["mean", "scale", "W_pos", "V_pos", "y", "theta_pos", "genes", "kind", "lognormal_mean"]
