"""CPU: everything tests/sparse_gaussian_cases.py builds -- the cases cover what they name, every probe is worth ten
tolerances in every output it feeds (fp64 oracle alone), the expanded sparse formulas equal the dense oracle -- and the
torch side of the sparse Gaussian path: ``SparseExpression``, ``log_normalize``, ``_init_gaussian``, every refusal and the
host-only plan query.  No GPU is used."""
import pytest
import torch

import gaussian_cases as GC
import sparse_gaussian_cases as S

NAMES = S.case_names()


@pytest.fixture(scope="module", autouse=True)
def _library():
    from gpzoo_amd import build
    build.build(force=False, verbose=False)


def small_counts(seed=3, D=12, N=30):
    g = torch.Generator().manual_seed(seed)
    y = torch.poisson(2.0 * torch.rand(D, N, generator=g), generator=g) * (torch.rand(D, N, generator=g) < 0.4)
    y[3] = 0.0
    y[:, 5] = 0.0
    y[0, 0], y[D - 1, N - 1] = 4.0, 2.0
    return y


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------

def test_the_list_of_cases():
    assert NAMES == ["Lt1", "Lt4", "Lt5", "Lt20", "Lt63", "Lt64", "chunks", "empties", "D1", "batch_B1", "batch_B137",
                     "descending", "offset50", "center_false"]
    for Lt in S.FACTORS:
        c = S.case("Lt%d" % Lt)
        assert c["z"].shape == (80, 130) and c["mean"].shape == (Lt, 130) and c["W"].shape == (80, Lt) and "idx" not in c


def test_parameters_follow_gaussian_cases():
    c = S.case("Lt20")
    p = GC.make_inputs(80, 130, 20, seed=c["seed"])
    for k in ("mean", "scale", "b", "sd"):
        assert torch.equal(c[k], p[k])
    assert torch.equal(c["W"], p["W"] / 20.0 ** 0.5)
    assert float(c["sd"].min()) == pytest.approx(0.05) and float(c["sd"].max()) == pytest.approx(3.0)


def test_z_is_log1p_of_thinned_counts():
    c = S.case("Lt20")
    z = c["z"]
    probes = torch.zeros_like(z, dtype=torch.bool)
    for d, n, _ in c["probes"]:
        probes[d, n] = True
    frac = float((z != 0).double().mean())
    assert 0.04 < frac < 0.12
    body = z[(z != 0) & ~probes]
    assert float(body.min()) > 0.0 and float(body.max()) < 4.0          # log1p(count / size factor): counts of 2 .. ~15 over 0.5 .. 2
    assert torch.allclose(c["offset"], z.double().mean(1), rtol=0, atol=1e-15)


def test_chunk_case_rows():
    C = S.chunk_length()
    assert C == S.plan(1037, 137, 80, 20, 5000)["gene_chunk"]
    c = S.case("chunks")
    lens = (c["z"] != 0).sum(1)
    want = {"C-1": C - 1, "C": C, "C+1": C + 1, "2C+1": 2 * C + 1, "full": 1037}
    for k, d in S.CHUNK_GENES.items():
        assert int(lens[d]) == want[k], k
    have = {(d, n) for d, n, _ in c["probes"]}
    assert {(0, 0), (79, 1036)} <= have
    for d in S.CHUNK_GENES.values():
        spots = torch.nonzero(c["z"][d]).flatten().tolist()
        for lo in range(0, len(spots), C):
            assert (d, spots[lo]) in have and (d, spots[min(lo + C, len(spots)) - 1]) in have


def test_degenerate_structure():
    c = S.case("empties")
    for d in S.EMPTY_ROWS:
        assert not bool(c["z"][d].any())
    for n in S.EMPTY_COLS:
        assert not bool(c["z"][:, n].any())
    assert 0 in S.EMPTY_ROWS and 79 in S.EMPTY_ROWS and 0 in S.EMPTY_COLS and 129 in S.EMPTY_COLS
    assert S.case("D1")["z"].shape == (1, 130) and S.case("D1")["W"].shape == (1, 5)


def test_batch_views():
    for name, B in S.BATCH_SIZES.items():
        c = S.case("batch_" + name)
        idx = c["idx"]
        assert idx.numel() == B == c["B"] and c["mean"].shape == (20, B) and idx.unique().numel() == B
        inside = torch.zeros(1037, dtype=torch.bool)
        inside[idx] = True
        for d in S.CHUNK_GENES.values():           # the long rows hold spots outside the batch, and some inside
            row = c["z"][d] != 0
            assert bool((row & ~inside).any())
        assert bool((c["z"][S.CHUNK_GENES["full"]] != 0)[idx].all())
    d = S.case("descending")["idx"]
    assert d.numel() == 70 and bool((d[1:] < d[:-1]).all()) and int(d[0]) == 129


def test_offsets():
    assert bool((S.case("offset50")["offset"] == 50.0).all())
    assert bool((S.case("center_false")["offset"] == 0.0).all())
    assert float(S.case("Lt4")["offset"].abs().min()) > 0.0


@pytest.mark.parametrize("name", NAMES)
def test_every_probe_is_worth_ten_tolerances_in_every_output(name):
    """Dropping or doubling any one probe moves the log-likelihood, sse[d], dmean[:, n], dW[d], db[d] and dsd[d] of the
    fp64 oracle by at least ten of the tolerances the GPU test applies.  Every probe is at least 300."""
    c = S.case(name)
    assert c["probes"] and all(v >= S.PROBE for _, _, v in c["probes"])
    assert len(S.batch_probes(c)) == len(c["probes"])
    for (d, n, v), s in zip(c["probes"], S.sharpness(c, S.reference(name))):
        print(name, (d, n, v), {k: round(x, 1) for k, x in s.items()})
        assert set(s) == set(S.OUTPUTS)
        assert min(s.values()) >= S.SHARP_NEED, (name, d, n, v, s)


@pytest.mark.parametrize("name", NAMES)
def test_expanded_formulas_equal_the_dense_oracle(name):
    """The sums over the stored entries plus the Gram terms, in fp64, against fp64 autograd of the dense closed form: to
    1e-6 of each output's tolerance (the two differ by fp64 rounding only), ss to rtol 1e-12."""
    c, want = S.case(name), S.reference(name)
    f, tol = S.sparse_formulas(c), S.tolerances(want)
    assert abs(f["value"] - want.value) <= 1e-6 * tol["value"]
    assert bool(((f["sse"] - want.sse).abs() <= 1e-6 * tol["sse"] + 1e-9 * want.sse_atol).all())
    for k in S.GRADS:
        share = float(((f["grads"][k] - want.grads[k]).abs() / tol[k]).max())
        assert share <= 1e-6, (k, share)
    ss = S.null_ss(c)
    assert bool(((f["ss"] - ss).abs() <= 1e-12 * ss.abs()).all())
    if name == "empties":
        assert all(float(ss[d]) == 0.0 for d in S.EMPTY_ROWS)
    if name == "batch_B1":
        assert bool((ss == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# SparseExpression and log_normalize
# ---------------------------------------------------------------------------------------------------------------------

def test_sparse_expression_members_views_and_to_dense():
    import gpzoo.likelihoods as li
    c = S.case("batch_B137")
    e = S.expression({k: v for k, v in c.items() if k != "idx"})
    assert isinstance(e, li.SparseExpression) and e.shape == (80, 1037) and e.device.type == "cpu" and not e.is_view
    assert e.nnz == int((c["z"] != 0).sum()) and e.offset.dtype == torch.float64 and e.offset.shape == (80,)
    assert e.to("cpu") is e and e.cpu() is e
    dense = e.to_dense()
    assert dense.dtype == torch.float32 and torch.equal(dense, (c["z"].double() - c["offset"][:, None]).float())
    v = e[:, c["idx"]]
    assert v.is_view and v.shape == (80, 137) and v.values.base is e.values and v.offset.data_ptr() == e.offset.data_ptr()
    assert v.values.base.col_val.data_ptr() == e.values.col_val.data_ptr()          # nothing is copied
    assert torch.equal(v.to_dense(), dense[:, c["idx"]])
    assert v.nnz == int((c["z"][:, c["idx"]] != 0).sum())
    with pytest.raises(TypeError, match="of a view"):
        v[:, torch.tensor([0, 1])]
    with pytest.raises(TypeError, match="1-D integer tensor"):
        e[:, 3]
    with pytest.raises(IndexError):
        e[:, torch.tensor([1, 1])]
    with pytest.raises(TypeError, match="SparseCounts-structured"):
        li.SparseExpression(c["z"], c["offset"])
    with pytest.raises(ValueError, match="offset"):
        li.SparseExpression(e.values, torch.zeros(3))
    assert not isinstance(e, li.SparseCounts)


def test_log_normalize_against_plain_torch_on_the_dense_matrix():
    import gpzoo.likelihoods as li
    import gpzoo.utilities as ut
    y = small_counts()
    D, N = y.shape
    counts = li.SparseCounts(y)
    sz = torch.as_tensor(ut.scanpy_sizefactors(counts.T)).reshape(-1)
    assert float(sz[5]) == 0.0                                              # a spot without counts: nothing is stored for it
    zd = torch.where(y > 0, torch.log1p(y.double() / sz.double()[None, :]), torch.zeros((), dtype=torch.float64)).float()
    e = ut.log_normalize(counts)
    assert isinstance(e, li.SparseExpression) and e.shape == (D, N)
    assert torch.equal(e.values.to_dense(), zd)                             # bit-equal values
    assert float((e.offset - zd.double().mean(1)).abs().max()) <= 1e-12
    for k in ("col_ptr", "col_gene", "row_ptr", "row_spot", "row_perm"):    # the index arrays are shared, only col_val is new
        assert getattr(e.values, k) is getattr(counts, k)
    assert e.values.col_val is not counts.col_val and torch.equal(counts.to_dense(), y)
    assert float(e.offset[3]) == 0.0
    assert bool((ut.log_normalize(counts, center=False).offset == 0).all())
    given = torch.linspace(0.0, 1.0, D)
    e2 = ut.log_normalize(counts, offset=given)
    assert torch.equal(e2.offset, given.double()) and torch.equal(e2.values.col_val, e.values.col_val)
    own = 0.5 + torch.arange(N, dtype=torch.float64) / N
    e3 = ut.log_normalize(counts, size_factors=own)
    assert torch.equal(e3.values.to_dense(), torch.log1p(y.double() / own[None, :]).float())
    with pytest.raises(ValueError, match="size factors"):
        ut.log_normalize(counts, size_factors=torch.ones(N + 1))
    with pytest.raises(ValueError, match="offset"):
        ut.log_normalize(counts, offset=torch.ones(D + 1))
    for bad in (counts[:, torch.tensor([1, 2])], y, e):
        with pytest.raises(TypeError, match="whole SparseCounts"):
            ut.log_normalize(bad)


def test_init_gaussian_from_a_sparse_expression_matches_the_dense_result():
    import gpzoo.gp as G
    import gpzoo.likelihoods as li
    import gpzoo.utilities as ut
    y = small_counts(seed=4)
    e = ut.log_normalize(li.SparseCounts(y))
    dense = e.to_dense()
    torch.manual_seed(0)
    a = li.FA(G.GaussianPrior(dense, L=3), e, L=3)
    torch.manual_seed(0)
    b = li.FA(G.GaussianPrior(dense, L=3), dense, L=3)
    assert torch.equal(a.W, b.W)
    assert float((a.b - b.b).abs().max()) <= 1e-6 and float((a.noise - b.noise).abs().max()) <= 1e-6
    assert float(torch.nn.functional.softplus(a.noise)[3]) == pytest.approx(1e-3, rel=2e-2)   # the constant gene: the floor
    with pytest.raises(TypeError, match="whole SparseExpression"):
        li.FA(G.GaussianPrior(dense, L=3), e[:, torch.tensor([0, 1, 2])], L=3)


def test_every_refusal():
    import gpzoo.gp as G
    import gpzoo.likelihoods as li
    import gpzoo.utilities as ut
    from gpzoo_amd import ops
    y = small_counts(seed=5)
    D, N = y.shape
    e = ut.log_normalize(li.SparseCounts(y))
    q = torch.distributions.Normal(torch.zeros(2, N), torch.ones(2, N))
    W, V, th = torch.ones(D, 2), torch.ones(N), torch.ones(D)
    with pytest.raises(TypeError, match="not counts"):
        li.poisson_expected_loglik([q], [W], V, e, E=2)
    with pytest.raises(TypeError, match="not counts"):
        li.nb_expected_loglik([q], [W], V, th, e, E=2)
    with pytest.raises(TypeError, match="not counts"):
        li.poisson_deviance([q], [W], V, e)
    with pytest.raises(TypeError, match="not counts"):
        li.nb_deviance([q], [W], V, th, e)
    with pytest.raises(TypeError, match="not counts"):
        ut.regularized_nmf(e, 2, solver="mu", beta_loss="kullback-leibler")
    with pytest.raises(TypeError, match="not counts"):
        ut.scanpy_sizefactors(e)
    with pytest.raises(TypeError, match="gaussian_fa_sparse"):
        ops.gaussian_fa(q.mean, q.scale, W, th, th, e)
    with pytest.raises(TypeError, match="normalised expression is dense"):
        ops.gaussian_fa(q.mean, q.scale, W, th, th, li.SparseCounts(y))        # unchanged
    with pytest.raises(TypeError, match="must be a SparseExpression"):
        ops.gaussian_fa_sparse(q.mean, q.scale, W, th, th, li.SparseCounts(y))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.gaussian_fa_sparse(q.mean, q.scale, W, th, th, e)
    model = li.FA(G.GaussianPrior(e.to_dense(), L=2), e, L=2)
    pY = model(E=2)[0]
    with pytest.raises(TypeError, match="to_dense"):
        pY.log_prob(e)
    assert pY.log_prob(e.to_dense()).shape == (2, D, N)
    with pytest.raises(TypeError, match="fused=True"):
        ut._fused_counts_only(model, e, False)
    ut._fused_counts_only(model, e, True)


def test_plan_query():
    from gpzoo_amd import _lib, ops
    p = ops.gaussian_fa_sparse_plan(1037, 137, 80, 20, 4000)
    assert set(p) == {"gene_chunk", "n_gene_chunks", "factors_padded", "workspace_bytes"}
    C = p["gene_chunk"]
    assert C >= 64 and p["n_gene_chunks"] == 80 + 4000 // C and p["factors_padded"] == 20 and p["workspace_bytes"] > 0
    assert [ops.gaussian_fa_sparse_plan(10, 10, 4, Lt, 0)["factors_padded"] for Lt in (1, 4, 5, 20, 63, 64)] == [4, 4, 8, 20, 64, 64]
    # nothing of D x B or nnz elements: at the Slide-seq mini-batch and 5 % density the scratch is a small fraction of either
    D, N, B, nnz = 17702, 39694, 7000, int(0.05 * 17702 * 39694)
    big = ops.gaussian_fa_sparse_plan(N, B, D, 20, nnz)
    assert big["workspace_bytes"] < 4 * nnz // 4 and big["workspace_bytes"] < 4 * D * B // 10
    more = ops.gaussian_fa_sparse_plan(N, B, D, 20, 2 * nnz)
    assert more["workspace_bytes"] - big["workspace_bytes"] <= (nnz // C + 1) * (20 + 4 + 1) * 8 + 4096
    with pytest.raises(ValueError, match="gpz_gaussian_fa_sparse: 65 factors unsupported"):
        ops.gaussian_fa_sparse_plan(10, 10, 4, 65, 0)
    with pytest.raises(ValueError, match="a batch of 11 distinct spots out of 10"):
        ops.gaussian_fa_sparse_plan(10, 11, 4, 3, 0)
    with pytest.raises(ValueError, match="bad extents"):
        ops.gaussian_fa_sparse_plan(10, 10, 0, 3, 0)
    lib = _lib.load()
    assert lib.gpz_gaussian_fa_sparse_plan(10, 10, 4, 3, 1 << 31, None, None, None, None) < 0
    assert b"32 bits" in lib.gpz_last_error()
