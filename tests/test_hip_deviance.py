"""GPU: the Poisson deviance entries (gpz_poisson_deviance, gpz_poisson_deviance_sparse; csrc/deviance.hip) against the
fp64 oracle of tests/deviance_cases.py, and ``deviance`` of the models.

The reference has no deviance function, so no reference run pins these outputs; the oracle is fp64 torch on the same
fp32 inputs through torch.distributions.Poisson (tests/test_deviance_cases.py checks it against the written-out formula,
the cases, and the sharpness of every probe on the CPU).

Bounds: the project's Poisson ones (poisson_cases.LL_REL / LL_ABS / G_RTOL / G_ATOL),

  total, sum_y, sum_mu, null_total          |got - ref| <= 5e-5 |ref| + 1e-3
  per_gene, per_spot, null_per_gene         |got - ref| <= 1e-3 |ref| + 1e-3 max|ref|

Tile and chunk boundaries come from the plan queries; none is restated.  Every comparison prints err / tolerance per
output before it asserts; with GPZ_TEST_RECORD_DIR set the figures are appended to deviance.jsonl there."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

import deviance_cases as DC
from helpers import record

pytestmark = pytest.mark.gpu

FLAGS = [True, False]


def dplan(N, D, Lt):
    from gpzoo_amd import ops
    return ops.poisson_deviance_plan(N, D, Lt)


def gene_chunk():
    from gpzoo_amd import ops
    return ops.poisson_deviance_sparse_plan(2000, 2000, 6, 5, 1000)["gene_chunk"]


def _params(c):
    return [c[k].float().cuda() for k in ("mean", "scale", "W", "V")]


def run_dense(c, flag=True):
    from gpzoo_amd import ops
    return ops.poisson_deviance(*_params(c), c["y"].float().cuda(), flag)


def counts_of(c):
    from gpzoo_amd.likelihoods import SparseCounts
    return SparseCounts(c["y"].float()).cuda()


def run_sparse(c, flag=True, counts=None):
    from gpzoo_amd import ops
    return ops.poisson_deviance_sparse(*_params(c), counts_of(c) if counts is None else counts, None, flag)


def check(c, got, flag, tag):
    ref = DC.oracle(c, flag)
    for k in DC.OUTPUTS:
        assert got[k].dtype == torch.float64 and not got[k].requires_grad, k
    fig = DC.figures(ref, got)
    print(tag, "lognormal" if flag else "plug-in", "err/tol", {k: f"{v:.3g}" for k, v in fig.items()})
    record("deviance.jsonl", dict(case=str(tag), lognormal_mean=flag, err_over_tol=fig), append=True)
    for k, v in fig.items():
        assert v <= 1.0, (tag, k, v)


def bits_equal(a, b):
    return all(torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)) for k in DC.OUTPUTS)


# --- 1. factor instances ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flag", FLAGS, ids=["lognormal", "plugin"])
@pytest.mark.parametrize("entry", ["dense", "sparse"])
@pytest.mark.parametrize("Lt", DC.FACTOR_COUNTS)
def test_factor_instances(Lt, entry, flag):
    c = DC.dense_case(130, 80, Lt, dplan(130, 80, Lt))
    check(c, run_dense(c, flag) if entry == "dense" else run_sparse(c, flag), flag, f"{entry}-Lt{Lt}")


# --- 2. tile edges (dense) -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("e", DC.EDGE_SPOTS, ids=lambda e: f"{e[0]}ts{e[1]:+d}")
def test_spot_tile_edges(e):
    """N one below, at and one above the plan's spots per tile, 1, two tiles + 1, and N no multiple of 4."""
    N = DC.edge(dplan(130, 80, 5)["spots_per_tile"], e)
    D = DC.ONE_SPOT_GENES if N == 1 else 37
    c = DC.dense_case(N, D, 5, dplan(N, D, 5))
    for flag in FLAGS:
        check(c, run_dense(c, flag), flag, f"N{N}")
        check(c, run_sparse(c, flag), flag, f"sparse-N{N}")


@pytest.mark.parametrize("unit,e", [("genes_per_tile", e) for e in DC.EDGE_GENES] + [("genes_per_block", e) for e in DC.EDGE_BLOCKS],
                         ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]:+d}")
def test_gene_tile_and_slice_edges(unit, e):
    """D one below, at and one above the plan's genes per tile and every gene-slice (workgroup block) boundary."""
    D = DC.edge(dplan(130, 80, 5)[unit], e)
    c = DC.dense_case(70, D, 5, dplan(70, D, 5))
    assert dplan(70, D, 5)["gene_slices"] == -(-D // dplan(70, D, 5)["genes_per_block"])
    for flag in FLAGS:
        check(c, run_dense(c, flag), flag, f"D{D}")


def test_spot_slices():
    """More than one spot slice: per-gene partial slabs added in slice order, probes on both sides of every slice cut."""
    p = dplan(*DC.SLICED)
    assert p["spot_slices"] > 1
    c = DC.dense_case(*DC.SLICED, p)
    check(c, run_dense(c), True, "sliced")
    check(c, run_sparse(c), True, "sparse-sliced")


def test_unaligned_counts_pointer():
    """y at an element offset that is no multiple of 16 bytes (a view): rows are then read element by element."""
    from gpzoo_amd import ops
    c = DC.dense_case(128, 37, 5, dplan(128, 37, 5))
    buf = torch.zeros(37 * 128 + 1, dtype=torch.float32, device="cuda")
    y = buf[1:].view(37, 128)
    y.copy_(c["y"].float())
    assert y.data_ptr() % 16 == 4
    check(c, ops.poisson_deviance(*_params(c), y, True), True, "unaligned-y")


# --- 3. zeros --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ["dense", "sparse"])
def test_all_zero_counts(entry):
    """total = 2 sum mu, the null deviance exactly 0, explained NaN."""
    from gpzoo_amd.likelihoods import SparseCounts, poisson_deviance
    c = DC.zeros_cases()["all_zero"]
    got = run_dense(c) if entry == "dense" else run_sparse(c)
    check(c, got, True, f"{entry}-all-zero")
    assert float(got["sum_y"]) == 0.0 and float(got["null_total"]) == 0.0 and bool((got["null_per_gene"] == 0).all())
    assert float(got["total"]) == pytest.approx(2.0 * float(got["sum_mu"]), rel=1e-6)
    mean, scale, W, V = _params(c)
    y = c["y"].float().cuda()
    r = poisson_deviance([torch.distributions.Normal(mean, scale)], [W], V, SparseCounts(y) if entry == "sparse" else y)
    assert bool(torch.isnan(r.explained)) and bool(torch.isnan(r.explained_per_gene).all())
    assert float(r.mean) == pytest.approx(float(got["total"]) / (c["D"] * c["N"]), rel=1e-12)


@pytest.mark.parametrize("entry", ["dense", "sparse"])
def test_a_gene_and_a_spot_without_counts(entry):
    c = DC.zeros_cases()["empty_gene_and_spot"]
    got = run_dense(c) if entry == "dense" else run_sparse(c)
    check(c, got, True, f"{entry}-empty-gene-and-spot")
    assert float(got["null_per_gene"][17]) == 0.0
    mu = DC.rate(c, True)
    # exactly the dense-term part: 2 sum mu over the row / the column
    assert float(got["per_gene"][17]) == pytest.approx(2.0 * float(mu[17].sum()), rel=1e-5)
    assert float(got["per_spot"][66]) == pytest.approx(2.0 * float(mu[:, 66].sum()), rel=1e-5)


# --- 4. sparse rows and columns --------------------------------------------------------------------------------------

def test_gene_chunk_boundaries():
    """Gene rows of exactly one chunk, one chunk + 1 and three chunks of non-zeros (length from the plan; columns are not
    split), probes at the first and last entry of every chunk; against the oracle and against the dense entry."""
    c = DC.chunk_case(gene_chunk())
    for flag in FLAGS:
        check(c, run_sparse(c, flag), flag, "chunks")
    check(c, run_dense(c), True, "chunks-dense")


def test_no_stored_values():
    """nnz = 0: every output is the dense term."""
    c = DC.zeros_cases()["all_zero"]
    counts = counts_of(c)
    assert counts.nnz == 0
    check(c, run_sparse(c, True, counts), True, "nnz0")


def test_every_value_stored():
    """A density of 100 %."""
    c = DC.make_probe_case(130, 80, 5, [(0, 0), (0, 129), (79, 0), (79, 129)], seed=8, edit=_at_least_one)
    counts = counts_of(c)
    assert counts.nnz == 130 * 80
    for flag in FLAGS:
        check(c, run_sparse(c, flag, counts), flag, "dense-100%")


def _at_least_one(y):
    y.clamp_(min=1.0)


# --- 5. views --------------------------------------------------------------------------------------------------------

def test_view_of_the_counts():
    """y[:, idx] with an unsorted idx of 37 of 130 spots that holds the first and last spot and leaves out a spot with a
    probe: the oracle on the dense columns, the dense entry on y.to_dense()[:, idx], per_spot in idx's order."""
    from gpzoo_amd import ops
    c, idx = DC.view_case()
    v = DC.view(c, idx)
    counts = counts_of(c)
    sub = counts[:, idx.cuda()]
    for flag in FLAGS:
        got = ops.poisson_deviance_sparse(*_params(v), sub, None, flag)
        check(v, got, flag, "view")
        same = ops.poisson_deviance_sparse(*_params(v), counts, idx.cuda(), flag)      # idx= is shorthand for the view
        assert bits_equal(got, same)
        dense = ops.poisson_deviance(*_params(v), counts.to_dense()[:, idx.cuda()], flag)
        check(v, dense, flag, "view-dense")
    assert got["per_spot"].shape == (37,)
    with pytest.raises(TypeError, match="view"):
        sub[:, torch.arange(3, device="cuda")]                                         # a view of a view still raises


def test_view_validation_is_deferred():
    from gpzoo_amd import ops
    c, idx = DC.view_case()
    v = DC.view(c, idx)
    bad = idx.clone()
    bad[3] = bad[4]                                                                    # a repeated spot
    counts = counts_of(c)
    with pytest.raises(IndexError, match="distinct"):
        ops.poisson_deviance_sparse(*_params(v), counts, bad.cuda(), True)
    reached = []
    with pytest.raises(IndexError, match="distinct"):
        with ops.deferred_info():
            ops.poisson_deviance_sparse(*_params(v), counts, bad.cuda(), True)
            reached.append(1)
    assert reached == [1]


# --- 6. dense against sparse, reproducibility ------------------------------------------------------------------------

def test_dense_against_sparse_on_the_same_counts():
    c = DC.make_probe_case(130, 80, 20, DC.dense_positions(130, 80, dplan(130, 80, 20)), seed=9, density=0.2)
    ref = DC.oracle(c)
    a, b = run_dense(c), run_sparse(c)
    check(c, a, True, "same-dense")
    check(c, b, True, "same-sparse")
    fig = DC.figures({k: a[k].cpu() for k in DC.OUTPUTS}, b)
    print("sparse against dense err/tol", fig)
    assert max(fig.values()) <= 1.0 and set(ref) == set(DC.OUTPUTS)


@pytest.mark.parametrize("entry", ["dense", "sparse"])
def test_two_calls_agree_bit_for_bit(entry):
    cases = [DC.dense_case(*DC.SLICED, dplan(*DC.SLICED))] if entry == "dense" else [DC.chunk_case(gene_chunk())]
    cases.append(DC.dense_case(130, 80, 20, dplan(130, 80, 20)))
    for c in cases:
        run = run_dense if entry == "dense" else run_sparse
        first = run(c)
        first = {k: first[k].clone() for k in DC.OUTPUTS}
        from gpzoo_amd import ops
        ops._workspace(torch.device("cuda", torch.cuda.current_device()), 1).fill_(0x5A)      # another workspace content
        assert bits_equal(first, run(c))


# --- 7. argument errors ----------------------------------------------------------------------------------------------

def test_argument_errors_launch_nothing():
    """Lt = 0 and 65, a null pointer, a workspace one byte short, a misaligned W or workspace: -1, gpz_last_error() set, and
    the outputs keep what they held (tests/test_deviance_api.py makes the same calls on the host alone)."""
    from gpzoo_amd import _lib
    lib = _lib.load()
    c = DC.dense_case(130, 80, 5, dplan(130, 80, 5))
    N, D, Lt = 130, 80, 5
    mean, scale, W, V = _params(c)
    y = c["y"].float().cuda()
    Wbuf = torch.zeros(D * Lt + 1, dtype=torch.float32, device="cuda")
    W_off = Wbuf[1:].view(D, Lt)
    outs = [torch.full((n,), -7.0, dtype=torch.float64, device="cuda") for n in (D, N, D, 4)]
    need = lib.gpz_poisson_deviance_workspace_bytes(N, D, Lt)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())                                             # noqa: E731

    def call(mean=mean, W=W, Lt=Lt, ws_ptr=ws.data_ptr(), ws_bytes=need):
        return lib.gpz_poisson_deviance(None if mean is None else P(mean), P(scale), P(W), P(V), P(y), N, D, Lt, 1,
                                        *(P(o) for o in outs), C.c_void_p(ws_ptr), ws_bytes, None)

    for kw, word in ((dict(Lt=0), "factors"), (dict(Lt=65), "factors"), (dict(mean=None), "null pointer"),
                     (dict(ws_bytes=need - 1), "workspace"), (dict(W=W_off), "aligned"), (dict(ws_ptr=ws.data_ptr() + 8), "aligned")):
        assert call(**kw) == -1, kw
        assert word in lib.gpz_last_error().decode(), kw
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs)
    assert call() == 0
    torch.cuda.synchronize()
    got = dict(zip(("per_gene", "per_spot", "null_per_gene"), outs[:3]))
    got.update(total=outs[3][0], sum_y=outs[3][1], sum_mu=outs[3][2], null_total=outs[3][3])
    check(c, got, True, "ctypes")

    counts = counts_of(c)
    need = lib.gpz_poisson_deviance_sparse_workspace_bytes(N, N, D, counts.nnz, Lt)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    outs = [torch.full((n,), -7.0, dtype=torch.float64, device="cuda") for n in (D, N, D, 4)]

    def call_sparse(mean=mean, W=W, Lt=Lt, ws_ptr=ws.data_ptr(), ws_bytes=need):
        return lib.gpz_poisson_deviance_sparse(None if mean is None else P(mean), P(scale), P(W), P(V), P(counts.col_ptr),
                                               P(counts.col_gene), P(counts.col_val), P(counts.row_ptr), P(counts.row_spot),
                                               P(counts.row_perm), None, None, N, N, D, counts.nnz, Lt, 1,
                                               *(P(o) for o in outs), C.c_void_p(ws_ptr), ws_bytes, None)

    for kw, word in ((dict(Lt=0), "factors"), (dict(Lt=65), "factors"), (dict(mean=None), "null pointer"),
                     (dict(ws_bytes=need - 1), "workspace"), (dict(W=W_off), "aligned"), (dict(ws_ptr=ws.data_ptr() + 8), "aligned")):
        assert call_sparse(**kw) == -1, kw
        assert word in lib.gpz_last_error().decode(), kw
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs)


# --- 8. models -------------------------------------------------------------------------------------------------------

N_M, M_M, D_M = 130, 20, 40


def _model_data():
    g = torch.Generator().manual_seed(71)
    X = 4.0 * torch.rand(N_M, 2, generator=g) - 2.0
    y = torch.poisson(2.0 * torch.rand(D_M, N_M, generator=g), generator=g)
    Xval = 4.0 * torch.rand(23, 2, generator=g) - 2.0
    yval = torch.poisson(2.0 * torch.rand(D_M, 23, generator=g), generator=g)
    Vval = 0.5 + torch.rand(23, generator=g)
    return g, X.cuda(), y.cuda(), Xval.cuda(), yval.cuda(), Vval.cuda()


def _build(kind, g, X, y):
    import gpzoo.gp as G
    import gpzoo.kernels as K
    from gpzoo.likelihoods import MGGP_NSF, NSF, Hybrid_NSF2
    L = 3
    Xc = X.cpu()
    if kind == "mggp_nsf":
        k = K.MGGP_NSF_RBF(sigma=1.0, lengthscale=2.0, group_diff_param=0.8, n_groups=2, L=L)
        gp = G.MGGP_WSVGP(k, dim=2, M=M_M, n_groups=2, jitter=1e-2)
        gp.groupsZ = nn.Parameter((torch.arange(M_M) % 2).long(), requires_grad=False)
    else:
        gp = G.WSVGP(K.NSF_RBF(L=L, lengthscale=2.0), dim=2, M=M_M, jitter=1e-2)
    gp.Z = nn.Parameter(Xc[:M_M].clone(), requires_grad=False)
    gp.mu = nn.Parameter(0.3 * torch.randn(L, M_M, generator=g))
    gp.Lu = nn.Parameter(0.05 * torch.randn(L, M_M, M_M, generator=g) - 0.5 * torch.eye(M_M))
    yc = y.cpu()
    if kind == "hybrid_nsf2":
        prior = G.GaussianPrior(yc, L=2)
        prior.mean = nn.Parameter(0.1 * torch.randn(2, N_M, generator=g))
        prior.scale = nn.Parameter(0.1 + 0.3 * torch.rand(2, N_M, generator=g))
        model = Hybrid_NSF2(gp, prior, yc, L=L, T=2)
        model.sf.W = nn.Parameter(torch.rand(D_M, L, generator=g))
        model.cf.W = nn.Parameter(torch.rand(D_M, 2, generator=g))
    else:
        model = (MGGP_NSF if kind == "mggp_nsf" else NSF)(gp, yc, L=L)
        model.W = nn.Parameter(torch.rand(D_M, L, generator=g))
    model.V = nn.Parameter(0.5 * torch.randn(N_M, generator=g))
    return model.cuda()


def _oracle_of(moments, W, V, y, flag=True):
    """The oracle applied to the model's own moments (rounded to fp32, as the entry sees them)."""
    f = lambda t: t.detach().float().double().cpu()                                    # noqa: E731
    c = dict(mean=torch.cat([f(q.mean) for q in moments]), scale=torch.cat([f(q.scale) for q in moments]),
             W=torch.cat([f(w) for w in W], dim=1), V=f(V), y=f(y))
    return c, DC.oracle(c, flag)


@pytest.mark.parametrize("kind", ["nsf", "mggp_nsf", "hybrid_nsf2"])
def test_model_deviance(kind):
    from gpzoo.likelihoods import PoissonDeviance
    from gpzoo_amd.likelihoods import SparseCounts
    sp = torch.nn.functional.softplus
    g, X, y, Xval, yval, Vval = _model_data()
    model = _build(kind, g, X, y)
    gX = (torch.arange(N_M, device="cuda") % 2).long()
    kw = dict(groupsX=gX) if kind == "mggp_nsf" else {}
    assert all(p.grad is None for p in model.parameters())
    r = model.deviance(X, y, **kw)
    assert isinstance(r, PoissonDeviance)
    assert all(isinstance(t, torch.Tensor) and t.dtype == torch.float64 and not t.requires_grad for t in r)
    assert all(p.grad is None for p in model.parameters())
    with torch.no_grad():
        if kind == "hybrid_nsf2":
            moments = [model.sf.prior(X=X)[0], model.cf.prior()[0]]
            W = [sp(model.sf.W), sp(model.cf.W)]
        elif kind == "mggp_nsf":
            moments, W = [model._gp(X, gX, False)[0]], [sp(model.W)]
        else:
            moments, W = [model.gp(X=X)[0]], [sp(model.W)]
    c, ref = _oracle_of(moments, W, sp(model.V), y)
    got = dict(per_gene=r.per_gene, per_spot=r.per_spot, null_per_gene=r.null_per_gene, total=r.total, sum_y=r.sum_y,
               sum_mu=r.sum_mu, null_total=r.null_total)
    fig = DC.figures(ref, got)
    print(kind, "err/tol", fig)
    assert max(fig.values()) <= 1.0
    assert float(r.explained) == pytest.approx(1.0 - float(ref["total"]) / float(ref["null_total"]), abs=1e-3)
    assert float(r.mean) == pytest.approx(float(ref["total"]) / (D_M * N_M), rel=1e-4)
    # a SparseCounts and a batch of it give the same numbers as the dense columns
    idx = torch.tensor([5, 129, 0, 77, 31, 64, 63], device="cuda")
    kwb = dict(groupsX=gX) if kind == "mggp_nsf" else {}
    rb = model.deviance(X, SparseCounts(y)[:, idx], idx=idx, **kwb)
    rd = model.deviance(X, y[:, idx], idx=idx, **kwb)
    assert rb.per_spot.shape == (7,)
    torch.testing.assert_close(rb.per_spot, rd.per_spot, rtol=2e-3, atol=0.0)
    torch.testing.assert_close(rb.total, rd.total, rtol=1e-4, atol=2e-3)
    # held-out spots
    kwv = dict(groupsX=(torch.arange(23, device="cuda") % 2).long()) if kind == "mggp_nsf" else {}
    if kind == "hybrid_nsf2":
        with pytest.raises(ValueError, match="fitted spots"):
            model.deviance(Xval, yval, V=Vval)
    else:
        with pytest.raises(ValueError, match="size factors"):
            model.deviance(Xval, yval, **kwv)
        rv = model.deviance(Xval, yval, V=Vval, **kwv)
        with torch.no_grad():
            qv = model._gp(Xval, kwv["groupsX"], False)[0] if kind == "mggp_nsf" else model.gp(X=Xval)[0]
        cv, refv = _oracle_of([qv], W, Vval, yval)
        figv = DC.figures(refv, dict(per_gene=rv.per_gene, per_spot=rv.per_spot, null_per_gene=rv.null_per_gene, total=rv.total,
                                     sum_y=rv.sum_y, sum_mu=rv.sum_mu, null_total=rv.null_total))
        print(kind, "held out err/tol", figv)
        assert max(figv.values()) <= 1.0
    assert all(p.grad is None for p in model.parameters())
