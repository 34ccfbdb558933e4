"""CPU: tests/gaussian_residual_cases.py -- the oracle, the fp32 emulation, the recorded tolerances, the redraw rule, the sparse
constructions and the planted case that tests/test_hip_gaussian_residual.py relies on."""
import numpy as np
import pytest
import torch

import gaussian_residual_cases as G

CASES = tuple(r[0] for r in G.TABLE)


def test_the_table_reaches_every_instance_and_both_thresholds():
    """All 13 k-step instances; the instance on either side of the prefetch threshold without the predictive kind (8 | 9
    k-steps) and with it (4 | 5), and of the split of the predictive kind's tile (10 | 12)."""
    steps = {G.K_STEPS[r[3]] for r in G.TABLE}
    assert steps == set(G.ALL_K_STEPS) and {4, 5, 8, 9, 10, 12} <= steps


@pytest.mark.parametrize("name", CASES)
def test_every_case_passes_within_three_draws_and_its_emulation_within_tolerance(name):
    c = G.make_case(name)
    assert 1 <= G.draws_used[name] <= G.MAX_DRAWS
    for kind in G.KINDS:
        fig = G.residual_figure(c, kind, G.emulate_residuals(c, kind))
        print(name, kind, "emulation err / tol", fig)
        assert fig <= 1.0 / 3.0
    wi, wc = G.stat_errors(c)
    assert wi <= G.I_ATOL / 3.0 and wc <= G.C_ATOL / 3.0


@pytest.mark.parametrize("name", CASES)
def test_inputs_are_what_the_issue_asks_for(name):
    c = G.make_case(name)
    assert (c["W"] > 0).any() and (c["W"] < 0).any() or c["W"].size == 1
    assert c["scale"].min() == 0.0 and 0.5 < c["scale"].max() < 1.5
    if c["D"] > 1:
        assert c["sd"].min() <= 1.01e-2 and c["sd"].max() >= 0.99e2
    for k in ("mean", "scale", "W", "b", "sd", "y"):
        assert np.array_equal(c[k], c[k].astype(np.float32).astype(np.float64))
    ref = G.oracle_residuals(c, "response")
    assert len(c["probes"]) >= 1
    for g, s, y in c["probes"]:
        assert abs(y) >= G.PROBE and abs(ref[g, s]) > 100.0 and np.sign(ref[g, s]) == np.sign(y)
    assert np.abs(G.predictive_mean(c)).max() < 30.0


def test_the_recorded_tolerances_are_three_times_the_measured_figures(capsys):
    """RTOL, CTOL, I_ATOL and C_ATOL are 3 x the worst emulated figure over seed 0 of the table, rounded up to one digit."""
    def up(v):
        e = 10.0 ** np.floor(np.log10(v))
        return float(np.ceil(v / e - 1e-9) * e)
    num = rel = wi = wc = 0.0
    for name, D, B, Lt, _ in G.TABLE:
        c = G._draw(name, D, B, Lt, 0)
        n, (r, _) = G.term_figures(c)
        i, cc = G.stat_errors(c)
        num, rel, wi, wc = max(num, n), max(rel, r), max(wi, i), max(wc, cc)
    assert np.isclose(G.CTOL, up(3 * num)) and np.isclose(G.RTOL, up(3 * rel))
    assert np.isclose(G.I_ATOL, up(3 * wi)) and np.isclose(G.C_ATOL, up(3 * wc))


@pytest.mark.parametrize("name", ["one_gene", "odd_small", "two_blocks", "lt20"])
def test_pearson_and_response_have_the_same_i_and_c(name):
    """The invariance under a per-gene affine map, in the oracle: to 1e-12."""
    c = G.make_case(name)
    nbr = G.case_table(c)
    a, b = G.spatial_stats(G.oracle_residuals(c, "pearson"), nbr), G.spatial_stats(G.oracle_residuals(c, "response"), nbr)
    assert np.abs(a["I"] - b["I"]).max() <= 1e-12 and np.abs(a["C"] - b["C"]).max() <= 1e-12
    assert np.allclose(a["kurtosis"], b["kurtosis"], rtol=1e-12)
    assert np.allclose(a["residual_var"] * c["sd"] ** 2, b["residual_var"], rtol=1e-12)
    p = G.spatial_stats(G.oracle_residuals(c, "predictive"), nbr)
    if c["D"] > 1:
        assert np.abs(p["I"] - a["I"]).max() > 1e-6          # another residual, another I


@pytest.mark.parametrize("name", ["odd_small", "lt20", "lt45"])
def test_predictive_is_pearson_where_q_is_a_point(name):
    c = G.make_case(name)
    point = (c["scale"] == 0).all(axis=0)
    assert point.any() and not point.all()
    for fn in (G.oracle_residuals, G.emulate_residuals):
        a, b = fn(c, "pearson"), fn(c, "predictive")
        assert np.array_equal(a[:, point], b[:, point]) and not np.array_equal(a[:, ~point], b[:, ~point])


@pytest.mark.parametrize("offset", G.OFFSETS)
@pytest.mark.parametrize("which", G.SPARSE_CASES)
def test_the_sparse_construction_is_to_dense_element_for_element(which, offset):
    c, v, off = G.sparse_case(which, offset)
    expr = G.sparse_expression(v, off)
    dense = expr.to_dense()
    assert dense.dtype == torch.float32 and np.array_equal(dense.double().numpy(), c["y"])
    lens = torch.diff(expr.values.row_ptr).tolist()
    if which == "rows":
        assert lens[1:4] == [511, 512, 513] and v[0, 599] != 0
    else:
        assert lens[17] == 0 and lens[64] == 130
    if offset == "uncentred":
        assert off[0] == 0.0 and off[1] == 50.0 and np.abs(v.mean(axis=1) - off).max() > 1.0
        assert (c["y"][1][v[1] == 0] == -50.0).all()
    else:
        assert np.abs((v - off[:, None]).mean(axis=1)).max() < 1e-12
    for kind in G.KINDS:
        assert G.residual_figure(c, kind, G.emulate_residuals(c, kind), y=c["y"]) <= 1.0 / 3.0


def test_the_planted_genes_have_the_smallest_p_values_in_the_oracle():
    c = G.planted_case()
    assert c["planted"].sum() == 10 and c["D"] == 100 and c["perms"].shape == (199, 400)
    assert all(sorted(p.tolist()) == list(range(400)) for p in c["perms"][:5])
    R = G.residuals(c, "pearson")
    pg, pl = G.permutation_pvalues(R, c["nbr"], c["perms"])
    assert G.planted_found(pg, c["planted"]) and G.planted_found(pl, c["planted"])
    assert pg[c["planted"]].max() == 1.0 / 200.0
