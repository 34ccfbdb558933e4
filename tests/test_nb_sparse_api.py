"""CPU: the host-side contract of gpz_nb_nsf_sparse -- the three symbols, the plan query without a device, the workspace's
size, the refusals before any launch -- and what stays as it was: ops.nb_nsf still refuses a SparseCounts."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gpz_nb_nsf_sparse", "gpz_nb_nsf_sparse_workspace_bytes", "gpz_nb_nsf_sparse_plan")
SLIDESEQ = dict(N=39694, B=7000, D=17702, Lt=20, E=3)


def test_entries_are_declared_and_bound():
    from gpzoo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpzoo_hip.h")).read()
    assert re.search(r"^#define GPZ_VERSION 212$", hdr, re.M)
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.exported_symbols() and getattr(lib, name)
    assert lib.gpz_version() == 212
    from gpzoo_amd import build
    assert "nb_sparse.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "nb_sparse.hip"))


def test_plan_query_needs_no_device():
    from gpzoo_amd import ops
    s = SLIDESEQ
    p = ops.nb_nsf_sparse_plan(s["N"], s["B"], s["D"], s["Lt"], s["E"], 35_000_000)
    assert p["gene_chunk"] > 0 and p["n_gene_chunks"] >= s["D"] + 35_000_000 // p["gene_chunk"]
    assert p["factors_padded"] == 20 and p["zero_factors_padded"] == 20
    assert p["gene_slices"] >= 1 and p["spot_slices"] >= 1
    assert p["samples_per_group"] == 3 and p["zero_samples_per_group"] == 3 and p["samples_per_call"] == 3
    q = ops.nb_nsf_sparse_plan(130, 130, 80, 64, 100, 0)
    assert q["samples_per_call"] == 32 and q["samples_per_group"] < 32 and q["zero_samples_per_group"] == 4
    for bad in ((0, 0, 80, 20, 3, 0), (130, 131, 80, 20, 3, 0), (130, 130, 0, 20, 3, 0), (130, 130, 80, 65, 3, 0),
                (130, 130, 80, 0, 3, 0), (130, 130, 80, 20, 0, 0), (130, 130, 80, 20, 3, -1), (-5, -5, 80, 20, 3, 0)):
        with pytest.raises(ValueError, match="gpz_nb_nsf_sparse_plan"):
            ops.nb_nsf_sparse_plan(*bad)


def test_workspace_holds_nothing_of_D_x_B_or_nnz_elements():
    from gpzoo_amd import _lib, ops
    s = SLIDESEQ
    p35 = ops.nb_nsf_sparse_plan(s["N"], s["B"], s["D"], s["Lt"], s["E"], 35_000_000)
    p70 = ops.nb_nsf_sparse_plan(s["N"], s["B"], s["D"], s["Lt"], s["E"], 70_000_000)
    assert 0 < p35["workspace_bytes"] < p70["workspace_bytes"] < s["D"] * s["B"] * 4
    # between 35 M and 70 M non-zeros only the per-chunk arrays grow: the chunk's gene (int32), its dW partial
    # (factors_padded fp32) and its four fp64 sums; three arrays, each rounded up to 256 bytes
    per_chunk = 4 + 4 * p35["factors_padded"] + 4 * 8
    grown = p70["n_gene_chunks"] - p35["n_gene_chunks"]
    assert grown == 35_000_000 // p35["gene_chunk"]
    assert p70["workspace_bytes"] - p35["workspace_bytes"] <= grown * per_chunk + 3 * 256
    # the first sample of a split and a full call: E enters through O(E Lt B) arrays only
    lib = _lib.load()
    one = lib.gpz_nb_nsf_sparse_workspace_bytes(s["N"], s["B"], s["D"], 35_000_000, s["Lt"], 1)
    assert 0 < one < p35["workspace_bytes"]


def _call(lib, over=None, ws_bytes=None, **shape):
    """gpz_nb_nsf_sparse with host buffers as stand-ins: every case here must be refused before any launch."""
    s = dict(N=130, B=130, D=80, nnz=50, Lt=20, E=3)
    s.update(shape)
    buf = (C.c_char * 4096)()
    p = C.c_void_p((C.addressof(buf) + 63) // 64 * 64)
    names = ("mean", "scale", "eps", "W", "V", "theta", "col_ptr", "col_gene", "col_val", "row_ptr", "row_spot", "row_perm",
             "idx", "pos")
    outs = ("loglik", "dmean", "dscale", "dW", "dV", "dtheta", "ws")
    a = {k: p for k in names + outs}
    a["idx"] = a["pos"] = None
    a.update(over or {})
    need = lib.gpz_nb_nsf_sparse_workspace_bytes(s["N"], s["B"], s["D"], s["nnz"], s["Lt"], s["E"])
    rc = lib.gpz_nb_nsf_sparse(*[a[k] for k in names], s["N"], s["B"], s["D"], s["nnz"], s["Lt"], s["E"], 1,
                               *[a[k] for k in outs], need if ws_bytes is None else ws_bytes, None)
    return rc, lib.gpz_last_error().decode()


def test_argument_errors_before_any_launch():
    from gpzoo_amd import _lib
    lib = _lib.load()
    assert lib.gpz_nb_nsf_sparse_workspace_bytes(130, 130, 80, 50, 20, 3) > 0
    for bad in ((130, 130, 80, 50, 65, 3), (130, 130, 80, 50, 0, 3), (-1, 130, 80, 50, 20, 3), (130, 130, -80, 50, 20, 3),
                (130, 130, 80, -1, 20, 3), (130, 0, 80, 50, 20, 3), (130, 130, 80, 50, 20, 0), (130, 130, 80, 50, 20, 33),
                (130, 200, 80, 50, 20, 3), (1 << 24, 1 << 24, 80, 50, 64, 1)):
        assert lib.gpz_nb_nsf_sparse_workspace_bytes(*bad) == 0, bad
        assert lib.gpz_last_error().decode().startswith("gpz_nb_nsf_sparse_workspace_bytes:"), bad
    assert "2 GiB" in lib.gpz_last_error().decode()             # the last one: exp(F) beyond the dense step's limit
    refused = [dict(Lt=65), dict(Lt=0), dict(N=-1), dict(D=-80), dict(nnz=-1), dict(E=0), dict(E=33), dict(B=0), dict(B=131),
               dict(B=70),                                            # a batch without idx / pos
               dict(ws_bytes=1024)]
    refused += [dict(over={k: None}) for k in ("mean", "scale", "eps", "W", "V", "theta", "col_ptr", "col_gene", "col_val",
                                               "row_ptr", "row_spot", "row_perm", "loglik", "dmean", "dscale", "dW", "dV",
                                               "dtheta", "ws")]
    buf = (C.c_char * 256)()
    odd = C.c_void_p((C.addressof(buf) + 63) // 64 * 64 + 4)
    refused += [dict(over={k: odd}) for k in ("mean", "W", "theta", "dtheta", "ws")]
    refused += [dict(over={"idx": odd}), dict(over={"pos": odd})]
    for kw in refused:
        rc, msg = _call(lib, **kw)
        assert rc < 0 and msg.startswith("gpz_nb_nsf_sparse:"), (kw, rc, msg)
    rc, msg = _call(lib, Lt=65)
    assert "65 factors unsupported" in msg


def test_python_refusals_without_a_device():
    from gpzoo_amd import ops
    from gpzoo_amd.likelihoods import SparseCounts
    y = torch.zeros(4, 6)
    y[1, 2] = 3.0
    z = torch.zeros(2, 6)
    # (__wrapped__: the function behind the decorator that looks for the tensors' CUDA device first)
    with pytest.raises(TypeError, match="SparseCounts"):
        ops.nb_nsf_sparse.__wrapped__(z, z, z[None], torch.ones(4, 2), torch.ones(6), torch.ones(4), y)
    # ops.nb_nsf is as it was: dense counts only, and its message says so
    with pytest.raises(TypeError, match="takes dense counts"):
        ops.nb_nsf.__wrapped__(z, z, z[None], torch.ones(4, 2), torch.ones(6), torch.ones(4), SparseCounts(y))


def test_nb_expected_loglik_chooses_by_the_counts():
    from gpzoo_amd import likelihoods as li
    y = torch.zeros(4, 6)
    y[1, 2] = 3.0
    s = li.SparseCounts(y)
    assert li._nb_loglik_function(y) is li._NBLogLik
    assert li._nb_loglik_function(s) is li._SparseNBLogLik and li._nb_loglik_function(s[:, torch.tensor([2, 0])]) is li._SparseNBLogLik
    assert "SparseCounts" in li.nb_expected_loglik.__doc__ and "raises TypeError" not in li.nb_expected_loglik.__doc__
    assert hasattr(li.PNMF, "expected_loglik")
