"""CPU: the numpy oracle of the sparse-GP gene test (tests/gene_gp_cases.py) checked against itself, and the conditions
the GPU comparison rests on asserted here, where a failure cannot hide behind an exemption.  No GPU is touched: the chunk
and tol_t come from the library's host-only plan queries."""
import math

import numpy as np
import pytest

import gene_gp_cases as GC

NAMES = sorted(GC.CASES)


def test_the_cases_cover_the_shapes_and_rows_the_kernels_branch_on():
    shapes = [GC.CASES[n] for n in NAMES]
    assert {s[0] for s in shapes} == {65, 257, 1037}
    assert {s[1] for s in shapes} == {8, 63, 64, 65, 129}
    assert {s[2] for s in shapes} == {1, 2, 3}
    assert {s[3] for s in shapes} == {1, 4, 9}
    assert {s[4] for s in shapes} == {"rbf", "matern32"}
    for n in NAMES:
        c = GC.build_case(n)
        V, N, chunk = c["V"], c["N"], c["chunk"]
        assert V.shape == (GC.D, N) and V.dtype == np.float32
        nnz = (V != 0).sum(axis=1)
        assert nnz[GC.EMPTY] == 0 and nnz[GC.ONE] == 1 and nnz[GC.HUGE] == 1 and nnz[GC.FULL] == N and nnz[GC.SMOOTH] == N
        assert np.all(V[GC.CONST] == V[GC.CONST, 0]) and V[GC.CONST, 0] != 0
        assert [nnz[g] for g in (GC.CHUNK_M1, GC.CHUNK_0, GC.CHUNK_P1)] == [min(chunk + k, N) for k in (-1, 0, 1)]
        assert chunk % 256 == 0
    assert any(GC.build_case(n)["N"] > GC.build_case(n)["chunk"] for n in NAMES)      # a row that is cut into chunks exists


@pytest.mark.parametrize("name", NAMES)
def test_conditions_the_gpu_comparison_rests_on(name):
    f = GC.oracle(name)["fit"]
    pairs = f["status"].size
    tied = int(f["near_tied"].sum())
    interior = int((f["status"] == 0).sum())
    print(f"{name}: {pairs} pairs, {tied} near-tied, {interior} interior")
    assert tied <= 0.02 * pairs
    assert interior >= pairs / 3
    assert np.all(f["status"][[GC.EMPTY, GC.CONST]] == 3)                       # degenerate after centring
    assert np.any(f["status"][GC.SMOOTH] == 2)                                   # the noise-free gene: delta at the lower bound


@pytest.mark.parametrize("name", NAMES)
def test_lr_is_not_negative_and_planted_genes_outrank_noise(name):
    o = GC.oracle(name)
    c, f = o["case"], o["fit"]
    lr = 2.0 * (f["F"] - o["null"][:, None])
    ok = f["status"] != 3
    # F(delta_max) stands in for the supremum: it lies below F_0 by at most the trace term (N - sum lam) / (2 delta_max) and
    # the first order of the other terms in 1 / delta_max, both below N / delta_max
    assert np.all(lr[ok] >= -2.0 * c["N"] / c["delta_range"][1])
    for l in set(c["planted_ell"].values()):
        planted = [lr[g, l] for g, at in c["planted_ell"].items() if at == l]
        assert min(planted) > max(lr[g, l] for g in GC.NOISE), (name, l)
    assert all(f["status"][g, l] == 0 for g, l in c["planted_ell"].items())      # strong enough for an interior optimum


@pytest.mark.parametrize("name", ["n257_m63_d2", "n257_m64_d3"])
def test_woodbury_form_against_the_dense_evaluation(name):
    o = GC.oracle(name)
    f = o["fit"]
    for g in (GC.FULL, GC.NOISE[2], GC.PLANTED[0], GC.PLANTED[4], GC.HUGE):
        for l in range(o["case"]["n_ell"]):
            dense = GC.dense_bound(name, g, l, f["s2"][g, l], f["tau2"][g, l])
            assert abs(dense - f["F"][g, l]) <= 1e-10 * abs(dense), (g, l, dense, f["F"][g, l])


@pytest.mark.parametrize("name", NAMES)
def test_the_bound_tends_to_the_null_model(name):
    o = GC.oracle(name)
    c = o["case"]
    for g in (GC.ONE, GC.FULL, GC.NOISE[0], GC.PLANTED[1]):
        for l in range(c["n_ell"]):
            F = float(GC.F_terms(math.log(1e13), o["p_ref"][l, g] ** 2, o["lam"][l], o["yty"][g], c["N"])[0])
            assert abs(F - o["null"][g]) <= 1e-9 * abs(o["null"][g]), (g, l)


def test_projections_of_a_case_against_fsum():
    o = GC.oracle("n257_m64_d3")
    c = o["case"]
    V = c["V"].astype(np.float64)
    rng = np.random.default_rng(5)
    for _ in range(200):
        l, g, m = rng.integers(c["n_ell"]), rng.integers(GC.D), rng.integers(c["M"])
        k = GC.kernel_matrix(c["kernel"], c["ell"][l], c["Z"][m:m + 1], c["X"])[0]
        want = math.fsum(float(v) * float(kk) for v, kk in zip(V[g], k) if v != 0)
        assert o["P_ref"][l, g, m] == want
    rtol_p, _ = GC.tolerances()
    assert np.all(np.abs(o["P_emu"] - o["P_ref"]) <= rtol_p * o["P_abs"])
    dense = np.einsum("gn,lmn->lgm", V, np.stack([GC.kernel_matrix(c["kernel"], e, c["Z"], c["X"]) for e in c["ell"]]))
    assert np.all(np.abs(dense - o["P_ref"]) <= 1e-12 * o["P_abs"] + 1e-300)


def test_tolerances_are_measured_and_of_the_size_of_the_arithmetic():
    rtol_p, rtol_f = GC.tolerances()
    print(f"RTOL_P = {rtol_p:.3e}, RTOL_F = {rtol_f:.3e}")
    eps = np.finfo(np.float64).eps
    assert eps < rtol_p < 1037 * eps             # a sequential sum of at most N terms
    assert 0 < rtol_f < 1e-6
    for n in NAMES:
        assert np.all(GC.delta_tolerance(n) >= 10 * GC.plan_tol_t(GC.CASES[n][1], GC.CASES[n][3]))
