"""CPU: the cases, probes and formulas of tests/sparse_nb_cases.py -- the decomposition of the negative-binomial step into
a zero part that reads no counts and a sum over the non-zeros against fp64 autograd through NegativeBinomial.log_prob, the
sharpness of every probe count, and the coverage of the case list against the library's plan query.  Nothing here needs a
GPU."""
import pytest
import torch

import nb_cases as NB
import poisson_cases as PC
import sparse_nb_cases as SN

CASES = SN.all_cases()
BY_NAME = dict(CASES)
PROBED = [(n, c) for n, c in CASES if c["probes"]]


@pytest.mark.parametrize("name,c", CASES, ids=[n for n, _ in CASES])
def test_decomposition_equals_the_oracle(name, c):
    """Zero part + non-zero part (plain torch, no autograd) against nb_cases.oracle: 1e-10 relative on the value and, for
    each gradient, 1e-10 of its largest entry.  (The largest figure is dtheta's at theta = 1e4, 8.2e-11: its terms cancel to
    O(1 / theta^2), and against 40-digit arithmetic the oracle and the formulas are each 3.3e-10 of max |dtheta| off there,
    mostly by the same amount -- torch's fp64 digamma, which both call with the same arguments.  Every other figure of
    every case is below 1e-11.)"""
    for with_lgamma in (False, True):
        (ref, grads), (got, g) = SN.reference(c, with_lgamma), SN.decomposed(c, with_lgamma)
        assert abs(got - ref) <= 1e-10 * abs(ref), (name, got, ref)
        for k in SN.GRADS:
            assert g[k].shape == grads[k].shape
            err, sc = float((g[k] - grads[k]).abs().max()), float(grads[k].abs().max())
            assert err <= 1e-10 * sc, (name, k, err / sc)


def test_decomposition_in_fp32_sits_inside_the_tolerances():
    """Plain fp32 torch on the same formulas: why nb_cases.check's tolerances need no loosening for this path."""
    c = SN.chunk_case()
    (ref, grads), (got, g) = SN.reference(c, True), SN.decomposed(c, True, dtype=torch.float32)
    assert abs(got - ref) <= 0.2 * SN.ll_tolerance(ref)
    for k in ("mean", "scale", "W", "V"):
        assert float(((g[k] - grads[k]).abs() / SN.tolerance(grads, k)).max()) <= 0.2, k


@pytest.mark.parametrize("name,c", PROBED, ids=[n for n, _ in PROBED])
def test_probes_are_sharp(name, c):
    """Every probe, none exempted: at most 20 000, and worth at least ten tolerances in the value (with and without the
    lgamma term), in its row of dW and in its entry of dV, by the fp64 oracle alone."""
    v = SN.dense_view(c)
    assert len(v["probes"]) == len(c["probes"]) >= 1
    for (d, n, cnt), s in zip(v["probes"], SN.sharpness(c)):
        assert v["y"][d, n] == cnt and 0 < cnt <= PC.COUNT_MAX
        assert set(s) == {"ll", "ll_lgamma", "dW", "dV"} and min(s.values()) >= PC.SHARP_NEED, (name, d, n, cnt, s)
    assert float(c["theta"].min()) > 0 and float(c["theta"].max()) <= SN.THETA_MAX


def test_probe_positions():
    C_ = SN.chunk_length()
    c = SN.chunk_case()
    lens = {k: int((c["y"][g] != 0).sum()) for k, g in SN.CHUNK_GENES.items()}
    assert C_ >= 2 and lens == {"C-1": C_ - 1, "C": C_, "C+1": C_ + 1, "2C+1": 2 * C_ + 1, "full": 1037}
    probes = {(d, n) for d, n, _ in c["probes"]}
    for g in SN.CHUNK_GENES.values():
        spots = torch.nonzero(c["y"][g]).reshape(-1).tolist()
        for lo in range(0, len(spots), C_):
            assert (g, spots[lo]) in probes and (g, spots[min(lo + C_, len(spots)) - 1]) in probes
    assert {(0, 0), (79, 1036)} <= probes
    for shape in SN.FACTOR_SHAPES + SN.SAMPLE_SHAPES:
        N, D = shape[:2]
        assert {(d, n) for d, n, _ in SN.shape_case(shape)["probes"]} == {(0, 0), (0, N - 1), (D - 1, 0), (D - 1, N - 1)}
    for shape in SN.TILE_SHAPES:
        N, D = shape[:2]
        assert {(0, 0), (D - 1, N - 1)} <= {(d, n) for d, n, _ in SN.tile_case(shape)["probes"]}
    col = SN.dense_column_case()
    assert SN.DENSE_COLUMN_SHAPE[1] == 2100 and bool((col["y"][:, SN.DENSE_COLUMN] != 0).all())
    assert {(0, SN.DENSE_COLUMN), (2099, SN.DENSE_COLUMN)} <= {(d, n) for d, n, _ in col["probes"]}


def test_every_kernel_instance_is_visited():
    """Against the plan query: the factor shapes and the tile-edge cases together reach every instance of the zero passes
    and of the non-zero passes that some factor count 1 .. 64 is served by."""
    every = [SN.plan(130, 130, 80, Lt, 3) for Lt in range(1, 65)]
    shapes = SN.FACTOR_SHAPES + SN.TILE_SHAPES
    seen = [SN.plan(N, N, D, Lt, E) for N, D, Lt, E in shapes]
    for key in ("zero_factors_padded", "factors_padded"):
        assert {p[key] for p in seen} == {p[key] for p in every}, key
    assert len({p["zero_factors_padded"] for p in every}) == 9 and len({p["factors_padded"] for p in every}) == 10
    assert sorted(s[2] for s in SN.FACTOR_SHAPES) == [1, 4, 5, 20, 33, 40, 63, 64]
    for N, D, Lt, E in shapes:
        p = SN.plan(N, N, D, Lt, E)
        assert p["factors_padded"] >= Lt and p["zero_factors_padded"] >= Lt and p["factors_padded"] % 4 == 0


def test_instance_end_shapes_reach_both_ends_of_every_zero_instance():
    every = {}
    for Lt in range(1, 65):
        every.setdefault(SN.plan(68, 68, 40, Lt, 2)["zero_factors_padded"], []).append(Lt)
    ends = sorted(Lt for v in every.values() for Lt in (min(v), max(v)))
    assert len(every) == 9 and sorted(s[2] for s in SN.INSTANCE_END_SHAPES) == ends
    for N, D, Lt, E in SN.INSTANCE_END_SHAPES:
        p = SN.plan(N, N, D, Lt, E)
        assert (N, D, E) == (68, 40, 2) and p["gene_slices"] == 1 and p["spot_slices"] == 1


def test_case_list_contains_each_boundary():
    # tile edges of the zero part
    assert {s[0] for s in SN.TILE_SHAPES} == set(NB.SPOTS) == {1, 63, 64, 65, 500}
    assert {s[1] for s in SN.TILE_SHAPES} == set(NB.GENES) == {1, 7, 130, 257}
    nd = {(s[0], s[1]) for s in SN.TILE_SHAPES}
    assert (500, 1) in nd                         # a single gene over many tiles
    assert (1, 257) in nd                         # a single spot under every gene block
    assert any(D % 16 for _, D in nd)             # a ragged 16-gene group
    assert any(D > 4 * 64 for _, D in nd)         # more than four 64-gene blocks
    for _, c in CASES:
        dens = float((c["y"] != 0).double().mean())
        assert dens <= 0.35 or c["y"].numel() <= 2100 * 66, dens
    # samples: more than one LDS group of the zero part's gene pass, and the host split
    assert [s[3] for s in SN.SAMPLE_SHAPES] == [1, 2, 5, 20, 33]
    p5, p33 = SN.plan(130, 130, 80, 7, 5), SN.plan(130, 130, 80, 7, 33)
    assert p5["zero_samples_per_group"] < 5 and p33["samples_per_call"] < 33
    # degenerate structure
    e = BY_NAME["empties"]["y"]
    assert all(not e[d].any() for d in (0, 41, 79)) and all(not e[:, n].any() for n in (0, 66, 67, 129))
    assert int((BY_NAME["nnz0"]["y"] != 0).sum()) == 0 and int((BY_NAME["nnz1"]["y"] != 0).sum()) == 1
    assert BY_NAME["1x1"]["y"].shape == (1, 1)
    z = BY_NAME["stored_zero"]
    assert len(z["stored_zeros"]) >= 1 and all(z["y"][d, n] == 0 for d, n in z["stored_zeros"])
    vals = BY_NAME["values"]["y"]
    assert bool((vals >= 256).any()) and bool((vals != vals.round()).any())
    big = BY_NAME["big_counts"]["y"]
    row = big[SN.BIG_ROW][big[SN.BIG_ROW] != 0]
    rest = torch.cat([big[:SN.BIG_ROW], big[SN.BIG_ROW + 1:]])
    assert float(rest[rest != 0].min()) >= 16.0 and len(row) >= 3 and bool((row != row.round()).all()) and float(row.min()) < 16.0
    # batches
    idx = SN.batch_indices()
    assert len(idx["B1"]) == 1 and len(idx["B70"]) == 70 and sorted(idx["perm"]) == list(range(1037))
    assert idx["B70"] != sorted(idx["B70"])
    ye = BY_NAME["batch_empty_cols"]
    assert all(not ye["y"][:, n].any() for n in SN.BATCH_EMPTY_COLS) and set(SN.BATCH_EMPTY_COLS) <= set(idx["empty_cols"])
    yh = BY_NAME["batch_hidden_gene"]
    assert bool(yh["y"][SN.BATCH_HIDDEN_GENE].any()) and not SN.batch_dense(yh)[SN.BATCH_HIDDEN_GENE].any()
    # the Poisson limit
    lim = BY_NAME["poisson_limit"]
    assert bool((lim["theta"] == 1e4).all()) and tuple(lim["y"].shape) == (37, 65) and lim["Lt"] == 5 and lim["E"] == 3
    assert bool((SN.poisson_limit_theta_atol(lim) > 0).all())


def test_theta_follows_nb_cases():
    c = SN.shape_case(SN.FACTOR_SHAPES[0])
    want = NB.make_inputs(80, 4, 1, 1, seed=0)["theta"].double()
    untouched = [d for d in range(80) if d not in (0, 79)]
    assert torch.equal(c["theta"][untouched], want[untouched])
    assert bool((c["theta"] >= want).all())                     # a probe's gene may only have been raised
