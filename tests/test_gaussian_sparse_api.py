"""CPU: the surface of the sparse Gaussian path -- the two C entries and their host-side refusals, the Python entry
points and the re-exports under the ``gpzoo`` names."""
import ctypes as C
import os
import re

import torch

from conftest import ROOT

NEW_SYMBOLS = ("gpz_gaussian_fa_sparse", "gpz_gaussian_fa_sparse_plan")


def header():
    return open(os.path.join(ROOT, "include", "gpzoo_hip.h")).read()


def test_new_entries_are_declared_exported_and_bound():
    from gpzoo_amd import _lib, build, ops
    hdr = header()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in hdr and name in _lib.exported_symbols()
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
    assert lib.gpz_version() == 212
    assert "#define GPZ_VERSION 212" in hdr
    comment = hdr[hdr.index("Additions under version 212"):hdr.index("#ifndef GPZOO_HIP_H")]
    assert all(n in comment for n in NEW_SYMBOLS)
    assert callable(ops.gaussian_fa_sparse) and callable(ops.gaussian_fa_sparse_plan)
    assert "gaussian_sparse.hip" in build.SOURCES                      # the source hash covers the new file
    assert os.path.exists(os.path.join(build.CSRC, "gaussian_sparse.hip"))


def test_scratch_is_the_explicit_argument_partials_sized_by_the_plan():
    """As for gpz_gaussian_fa: the scratch memory is the caller's ``partials`` and its size comes from the plan query."""
    hdr = header()
    args = re.search(r"\bgpz_gaussian_fa_sparse\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in args.replace("\n", " ").split(",")]
    assert names[:6] == ["mean", "scale", "W", "b", "noise_sd", "offset"]
    assert names[6:14] == ["col_ptr", "col_gene", "col_val", "row_ptr", "row_spot", "row_perm", "idx", "pos"]
    assert names[14:19] == ["N", "B", "D", "nnz", "Lt"]
    assert names[19:] == ["loglik", "sse_per_gene", "ss_per_gene", "dmean", "dscale", "dW", "db", "dnoise_sd", "partials",
                          "partials_bytes", "stream"]
    plan = re.search(r"\bgpz_gaussian_fa_sparse_plan\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in plan.replace("\n", " ").split(",")] == \
        ["N", "B", "D", "Lt", "nnz", "gene_chunk", "n_gene_chunks", "factors_padded", "workspace_bytes"]


def test_reexports_under_the_gpzoo_names():
    import gpzoo.likelihoods as li
    import gpzoo.utilities as ut
    import gpzoo_amd.likelihoods as ali
    import gpzoo_amd.utilities as aut
    assert li.SparseExpression is ali.SparseExpression and ut.log_normalize is aut.log_normalize
    assert callable(li.gaussian_expected_loglik) and callable(li.gaussian_score)
    assert issubclass(li._SparseGaussianFALogLik, torch.autograd.Function)
    assert li._gaussian_loglik_function(torch.zeros(2, 2)) is li._GaussianFALogLik
    e = ut.log_normalize(li.SparseCounts(torch.eye(3)))
    assert li._gaussian_loglik_function(e) is li._SparseGaussianFALogLik
    assert li._gaussian_loglik_function(e[:, torch.tensor([0, 2])]) is li._SparseGaussianFALogLik


def test_bad_arguments_are_refused_before_any_launch():
    from gpzoo_amd import _lib
    lib = _lib.load()
    null = [None] * 14
    rc = lib.gpz_gaussian_fa_sparse(*null, 10, 10, 4, 5, 3, *([None] * 9), 0, None)
    assert rc < 0 and b"gpz_gaussian_fa_sparse: null pointer" in lib.gpz_last_error()
    # host memory stands in for device memory: every refusal below comes before the first launch
    buf = (C.c_char * 8192)()
    base = (C.addressof(buf) + 15) & ~15
    p = lambda off=0: C.c_void_p(base + off)  # noqa: E731
    ok = [p(256 * i) for i in range(12)]

    def call(inputs=ok, idx=None, pos=None, N=10, B=10, D=4, nnz=5, Lt=3, ll=p(4096), grads=(None,) * 5, scratch=p(6144),
             nbytes=1 << 24):
        return lib.gpz_gaussian_fa_sparse(*inputs, idx, pos, N, B, D, nnz, Lt, ll, None, None, *grads, scratch, nbytes, None)
    assert call(ll=None) < 0 and b"null pointer" in lib.gpz_last_error()
    assert call(grads=(p(4352), None, None, None, None)) < 0 and b"all null or all set" in lib.gpz_last_error()
    assert call(Lt=65) < 0 and b"gpz_gaussian_fa_sparse: 65 factors unsupported (1..64)" in lib.gpz_last_error()
    assert call(N=0) < 0 and b"bad extents" in lib.gpz_last_error()
    assert call(B=11) < 0 and b"a batch of 11 distinct spots out of 10" in lib.gpz_last_error()
    assert call(B=5) < 0 and b"needs idx and pos" in lib.gpz_last_error()
    assert call(B=5, idx=p(4608)) < 0 and b"idx and pos come together" in lib.gpz_last_error()
    assert call(inputs=ok[:7] + [None] + ok[8:]) < 0 and b"null pointer (non-zeros)" in lib.gpz_last_error()
    assert call(scratch=p(6148)) < 0 and b"16-byte aligned" in lib.gpz_last_error()
    assert call(inputs=ok[:5] + [p(1284)] + ok[6:]) < 0 and b"8-byte aligned" in lib.gpz_last_error()
    assert call(nbytes=16) < 0 and b"partials too small" in lib.gpz_last_error()
    assert call(nnz=1 << 31) < 0 and b"32 bits" in lib.gpz_last_error()
