"""CPU: what the sparse-count KL NMF (gpz_nmf_kl_sparse_*, gpz_counts_matmul, SparseCounts.T, the sparse branch of
regularized_nmf and scanpy_sizefactors) can show without a GPU -- the host-only plan and workspace queries, argument
errors, the transposed view, the host paths of the two utilities, and that every case of tests/sparse_nmf_cases.py has the
structure the GPU tests rely on."""
import ctypes as C

import numpy as np
import pytest
import torch

import nmf_oracle as O
import sparse_nmf_cases as SC

SLIDESEQ = dict(N=39_694, D=17_702, nnz=35_000_000, L=20)


def test_plan_is_host_only_and_consistent():
    pads = [SC.plan(L=L)["factors_padded"] for L in range(1, 65)]
    assert all(p >= L for p, L in zip(pads, range(1, 65)))
    assert pads == sorted(pads) and pads[-1] == 64 and all(p % 4 == 0 for p in pads)    # 16-byte rows in fp32
    assert set(pads) == set(SC.instance_boundaries())
    p = SC.plan(**SLIDESEQ)
    assert p["gene_chunk"] >= 64 and p["spot_chunk"] >= 0 and p["colsum_rows"] >= 1
    assert p["n_gene_chunks"] >= SLIDESEQ["D"] + SLIDESEQ["nnz"] // p["gene_chunk"]       # an upper bound of sum ceil(len / c)
    assert SC.plan(**SLIDESEQ, dtype=torch.float64)["workspace_bytes"] > p["workspace_bytes"]
    for L in SC.boundary_factors():
        assert 1 <= L <= 64


def test_workspace_condition_at_slideseq_size():
    """No N x D array and nothing of nnz elements beyond the chunk list: under 128 MiB where the dense X is 2.8 GB."""
    nbytes = SC.plan(**SLIDESEQ)["workspace_bytes"]
    print(f"workspace at Slide-seq size, fp32: {nbytes / 2 ** 20:.1f} MiB")
    assert 0 < nbytes < 128 * 2 ** 20
    assert nbytes < SLIDESEQ["nnz"] * 4                                                   # less than one fp32 per non-zero


BAD_SHAPES = [dict(L=0), dict(L=65), dict(N=0), dict(D=0), dict(nnz=-1), dict(N=2 ** 31), dict(D=2 ** 31), dict(nnz=2 ** 31),
              dict(dtype=7)]


@pytest.mark.parametrize("bad", BAD_SHAPES, ids=lambda b: "-".join(f"{k}{v}" for k, v in b.items()))
def test_workspace_query_returns_zero_for_refused_arguments(bad):
    from gpzoo_amd import _lib
    lib = _lib.load()
    a = dict(N=100, D=50, nnz=500, L=5, dtype=_lib.GPZ_F32)
    assert lib.gpz_nmf_kl_sparse_workspace_bytes(a["N"], a["D"], a["nnz"], a["L"], a["dtype"]) > 0
    a.update(bad)
    assert lib.gpz_nmf_kl_sparse_workspace_bytes(a["N"], a["D"], a["nnz"], a["L"], a["dtype"]) == 0
    assert lib.gpz_last_error()
    assert lib.gpz_nmf_kl_sparse_plan(a["N"], a["D"], a["nnz"], a["L"], a["dtype"], None, None, None, None, None) < 0


def test_matmul_workspace_query_returns_zero_for_refused_arguments():
    from gpzoo_amd import _lib
    lib = _lib.load()
    assert lib.gpz_counts_matmul_workspace_bytes(100, 50, 500, 128, 1) > 0
    assert lib.gpz_counts_matmul_workspace_bytes(100, 50, 500, 1, 0) > 0
    for N, D, nnz, k, tr in [(100, 50, 500, 0, 0), (100, 50, 500, 129, 1), (0, 50, 500, 4, 0), (100, 2 ** 31, 500, 4, 0),
                             (100, 50, 2 ** 31, 4, 1), (100, 50, 500, 4, 2)]:
        assert lib.gpz_counts_matmul_workspace_bytes(N, D, nnz, k, tr) == 0, (N, D, nnz, k, tr)
        assert lib.gpz_last_error()


def test_entries_reject_bad_arguments_on_the_host():
    """rc < 0 and a message, before any launch: null pointers, L, k, extents, dtype, a small or misaligned workspace.  The
    pointers are host arrays that are never dereferenced."""
    from gpzoo_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    odd = C.c_void_p(p.value + 4)
    six = [p] * 6
    big = 1 << 30

    def upd(six=six, W=p, H=p, N=10, D=5, nnz=7, L=3, dt=_lib.GPZ_F32, iters=1, ws=p, nb=big):
        return lib.gpz_nmf_kl_sparse_update(*six, W, H, N, D, nnz, L, dt, iters, ws, nb, None)

    def div(six=six, W=p, H=p, N=10, D=5, nnz=7, L=3, dt=_lib.GPZ_F64, out=p, ws=p, nb=big):
        return lib.gpz_nmf_kl_sparse_divergence(*six, W, H, N, D, nnz, L, dt, out, ws, nb, None)

    def mm(six=six, Q=p, out=p, N=10, D=5, nnz=7, k=4, tr=0, ws=p, nb=big):
        return lib.gpz_counts_matmul(*six, Q, out, N, D, nnz, k, tr, ws, nb, None)

    calls = [(upd, dict(W=None), b"null"), (upd, dict(H=None), b"null"), (upd, dict(ws=None), b"null"),
             (upd, dict(six=[None] + six[1:]), b"null"), (upd, dict(six=six[:2] + [None] + six[3:]), b"null"),
             (upd, dict(L=0), b"L=0"), (upd, dict(L=65), b"L=65"), (upd, dict(N=2 ** 31), b"32 bits"),
             (upd, dict(D=2 ** 31), b"32 bits"), (upd, dict(nnz=2 ** 31), b"32 bits"), (upd, dict(dt=5), b"dtype"),
             (upd, dict(iters=0), b"iters"), (upd, dict(nb=64), b"workspace"), (upd, dict(ws=odd), b"aligned"),
             (div, dict(out=None), b"null"), (div, dict(W=None), b"null"), (div, dict(L=65), b"L=65"), (div, dict(dt=-1), b"dtype"),
             (div, dict(nb=64), b"workspace"), (div, dict(ws=odd), b"aligned"), (div, dict(six=six[:3] + [None] + six[4:]), b"null"),
             (mm, dict(Q=None), b"null"), (mm, dict(out=None), b"null"), (mm, dict(k=0), b"k=0"), (mm, dict(k=129), b"k=129"),
             (mm, dict(tr=3), b"transpose"), (mm, dict(tr=1, nb=64), b"workspace"), (mm, dict(ws=odd), b"aligned"),
             (mm, dict(N=2 ** 31), b"32 bits"), (mm, dict(six=six[:5] + [None]), b"null")]
    for fn, kw, word in calls:
        rc = fn(**kw)
        msg = lib.gpz_last_error()
        assert rc < 0 and word in msg, (fn.__name__, kw.keys(), rc, msg)


def test_transposed_view_round_trips():
    from gpzoo_amd.likelihoods import SparseCounts, TransposedCounts
    X = SC.named("small")["X"]
    counts = SC.counts_of(X)
    t = counts.T
    assert isinstance(t, TransposedCounts) and t.shape == X.shape and counts.shape == X.shape[::-1]
    assert t.T is counts and t.T.T.T is counts
    assert t.device == counts.device and t.nnz == counts.nnz == int((X != 0).sum())
    assert torch.equal(t.to_dense(), torch.as_tensor(X, dtype=torch.float32))
    assert t.dtype == torch.float32 and t.double().dtype == torch.float64 and t.double().float().dtype == torch.float32
    assert t.double().T is counts and t.float() is t and t.cpu() is t and t.to("cpu").T is counts
    assert t.double().T.col_val is counts.col_val                                          # no counts are copied
    with pytest.raises(TypeError, match="view"):
        counts[:, torch.arange(5)].T
    with pytest.raises(TypeError):
        TransposedCounts(counts[:, torch.arange(5)])
    assert isinstance(SparseCounts(t.T), SparseCounts)


def test_sizefactors_of_the_view_equal_the_dense_ones():
    from gpzoo.utilities import scanpy_sizefactors
    X = SC.named("small")["X"]
    e_spot = SC.named("small")["claims"]["empty"][0]
    assert not X[e_spot].any()
    got = scanpy_sizefactors(SC.counts_of(X).T)
    want = scanpy_sizefactors(X)
    assert isinstance(got, np.ndarray) and got.shape == (X.shape[0], 1) and got.dtype == np.float64
    assert got[e_spot, 0] == 0.0
    np.testing.assert_allclose(got, want, rtol=4 * np.finfo(np.float64).eps, atol=0)


def test_regularized_nmf_refuses_untransposed_counts():
    from gpzoo.utilities import regularized_nmf, scanpy_sizefactors
    counts = SC.counts_of(SC.named("small")["X"])
    kw = dict(solver="mu", beta_loss="kullback-leibler", init="random", max_iter=5)
    with pytest.raises(TypeError, match=r"\.T"):
        regularized_nmf(counts, 3, **kw)
    with pytest.raises(TypeError, match=r"\.T"):
        scanpy_sizefactors(counts)


def test_regularized_nmf_postprocessing_of_given_factors_needs_no_gpu():
    from gpzoo.utilities import regularized_nmf
    case = SC.named("small")
    X = case["X"]
    rng = np.random.default_rng(0)
    eF, Wl = rng.random((X.shape[0], 3)) + 0.1, rng.random((X.shape[1], 3)) + 0.1
    F, W = regularized_nmf(SC.counts_of(X).T, 3, factors=eF, loadings=Wl)
    Fo, Wo = O.postprocess(eF, Wl, 3)
    np.testing.assert_allclose(F, Fo, rtol=1e-12)
    np.testing.assert_allclose(W, Wo, rtol=1e-12)


def test_ops_reject_views_and_other_objects_before_touching_a_device():
    from gpzoo_amd import ops
    counts = SC.counts_of(SC.named("small")["X"])
    W, H = torch.ones(63, 3), torch.ones(3, 17)
    for fn in (lambda c: ops.nmf_kl_mu_sparse.__wrapped__(c, W, H), lambda c: ops.nmf_kl_divergence_sparse.__wrapped__(c, W, H),
               lambda c: ops.counts_matmul.__wrapped__(c, torch.ones(17, 2, dtype=torch.float64))):
        with pytest.raises(TypeError, match="view"):
            fn(counts[:, torch.arange(5)])
        with pytest.raises(TypeError, match="SparseCounts"):
            fn(torch.ones(17, 63))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.nmf_kl_mu_sparse.__wrapped__(counts, W, H)


@pytest.mark.parametrize("name", SC.names())
def test_case_has_the_structure_it_claims_and_the_oracle_stays_finite(name):
    case = SC.named(name)
    checked = SC.check_structure(case)
    X, W, H = case["X"], case["W0"].copy(), case["H0"].copy()
    counts = SC.counts_of(X)
    assert counts.shape == X.shape[::-1] and counts.nnz == int((X != 0).sum())
    assert torch.equal(counts.T.to_dense().double(), torch.as_tensor(X))                  # the counts hold exactly X
    lens = torch.diff(counts.row_ptr)
    for g, m in case["claims"].get("gene_lengths", []):
        assert int(lens[g]) == m
    for _ in range(10):
        W = O.update_w(X, W, H)
        H = O.update_h(X, W, H)
    assert np.isfinite(W).all() and np.isfinite(H).all() and np.isfinite(O.kl_divergence(X, W, H))
    print(f"{name}: X {X.shape}, nnz {counts.nnz} ({counts.nnz / X.size:.1%}), {checked} forced properties")
    assert checked >= (0 if name == "one" else 1)


def test_the_named_cases_cover_every_branch_the_plan_reports():
    p = SC.plan()
    c = p["gene_chunk"]
    assert sorted(m for _, m in SC.named("chunked")["claims"]["gene_lengths"]) == [c, c + 1, 2 * c + 1]
    assert SC.named("chunked")["X"].shape == (2 * c + 2, 40)
    assert SC.named("colsum_block")["X"].shape[0] == p["colsum_rows"] + 1
    D = SC.named("lanes_wrap")["X"].shape[1]
    assert D % 64 == 1 and D > 64 and (SC.named("lanes_wrap")["X"][1] > 0).all()
    assert ("spot_chunked" in SC.names()) == (p["spot_chunk"] > 0)
    for b in SC.instance_boundaries():
        assert f"L{b}" in SC.names() and (b == 64 or f"L{b + 1}" in SC.names())
        assert SC.plan(L=b)["factors_padded"] == b and (b == 64 or SC.plan(L=b + 1)["factors_padded"] > b)
