"""CPU: the oracles, the recorded tolerance and the planted conditions of tests/residual_perm_cases.py, which
tests/test_hip_residual_perm.py relies on."""
import numpy as np
import pytest
import torch

import geary_cases as Y
import moran_perm_cases as M
import residual_cases as R
import residual_perm_cases as Q


def _res(name="odd_small", kind="deviance", family="nb"):
    c = R.make_case(name)
    return c, R.oracle_residuals(c, kind, family)


def test_geary_and_kurtosis_written_out():
    """geary_c and kurtosis against plain loops over one small array."""
    c, res = _res("one_gene", "pearson", "poisson")
    res = np.vstack([res, np.arange(7.0)[None, :] ** 2])
    nbr = Y.ENUM_TABLES["irregular"]
    B, K = nbr.shape
    for g, x in enumerate(res):
        z = x - x.mean()
        G = sum((z[i] - z[j]) ** 2 for i in range(B) for j in nbr[i])
        assert Q.geary_c(res, nbr)[g] == pytest.approx((B - 1) * G / (2 * B * K * (z * z).sum()), rel=1e-13)
        assert Q.kurtosis(res)[g] == pytest.approx((z ** 4).mean() / (z ** 2).mean() ** 2, rel=1e-13)
    s = Q.stats(res, nbr)
    assert set(s) == {"I", "C", "mean", "var", "kurtosis"} and all(v.shape == (2,) for v in s.values())
    np.testing.assert_allclose(s["var"], res.var(axis=1), rtol=1e-13)
    assert np.isnan(Q.geary_c(np.ones((1, 7)), nbr)).all()


@pytest.mark.parametrize("name", ["odd_small", "long_rows"])
def test_the_relabelled_table_scores_what_the_permuted_array_scores(name):
    """T_pi[pi[i], m] = pi[nbr[i, m]]: the unpermuted residuals over T_pi give I and C of the permuted residuals over nbr."""
    c, res = _res(name)
    nbr = R.case_table(c)
    perms = Q.perms_of(c["B"], 4)
    assert (perms[0] == np.arange(c["B"])).all() and all(sorted(p) == list(range(c["B"])) for p in perms)
    I, C = Q.perm_stats(res, nbr, perms)
    for p, pi in enumerate(perms):
        T = M.relabelled(nbr, pi)
        assert (T[pi] == pi[nbr]).all()
        Ir, Cr = Q.relabelled_stats(res, nbr, pi)
        np.testing.assert_allclose(Ir, I[:, p], rtol=0, atol=1e-13)
        np.testing.assert_allclose(Cr, C[:, p], rtol=0, atol=1e-12)
    np.testing.assert_allclose(I[:, 0], R.morans_i(res, nbr)[0], rtol=0, atol=1e-13)       # the identity row (a copy: numpy may
    np.testing.assert_allclose(C[:, 0], Q.geary_c(res, nbr), rtol=0, atol=1e-13)           # add its elements in another order)
    assert np.abs(I[:, 1:] - I[:, :1]).max() > 1e-3          # a relabelling does change the statistic


def test_counts_bracket():
    obs = np.array([0.5, 1.0])
    sims = np.array([[0.5, 0.5 + 1e-10, 0.7, 0.1], [1.0 - 3e-10, 2.0, 2.0, 1.0]])
    ge, le, band = Q.counts_bracket(obs, sims)
    assert ge.tolist() == [1, 2] and le.tolist() == [1, 1] and band.tolist() == [2, 1]
    assert Q.BAND == 2e-10 == M.BAND and Q.MORAN_ATOL == 1e-10


def test_c_atol_is_three_times_the_measured_worst_error():
    worst, where = Q.c_error_worst()
    print("worst |C(emulated) - C(oracle)|", worst, where)
    assert where == "lt56 deviance poisson"
    assert 0.0 < worst <= Q.C_ATOL / 3.0
    assert Q.C_ATOL == 2e-6 and 3.0 * worst > Q.C_ATOL / 10.0           # one significant digit above three times the worst
    assert f"{worst:.2e}" in Q.__doc__ and "C_ATOL = 2e-6" in Q.__doc__


def test_the_enumeration_case_and_its_moments():
    """Five genes on seven spots; over all 5040 relabellings the mean and variance of I and C are the analytic randomisation
    moments at each gene's kurtosis, and the normality variance is visibly another number."""
    from gpzoo_amd.utilities import _autocorr_moments
    c = Q.enum_case()
    assert (c["D"], c["B"], c["Lt"]) == (5, 7, 1) and Y.enum_perms().shape == (5040, 7)
    res = R.oracle_residuals(c, "pearson", "poisson")
    for table, nbr in Y.ENUM_TABLES.items():
        assert nbr.shape[1] < 6                                          # not the complete graph, where both are constant
        e = Q.enum_moments(res, nbr)
        m = _autocorr_moments(torch.as_tensor(nbr), torch.as_tensor(Q.kurtosis(res)))
        np.testing.assert_allclose(e["EI"], float(m["EI"]), rtol=1e-11)
        np.testing.assert_allclose(e["EC"], 1.0, rtol=1e-11)
        np.testing.assert_allclose(e["VI"], m["VI_rand"].numpy(), rtol=1e-10)
        np.testing.assert_allclose(e["VC"], m["VC_rand"].numpy(), rtol=1e-10)
        for V in ("VI", "VC"):
            assert np.abs(e[V] / float(m[V + "_norm"]) - 1.0).max() >= 0.05, (table, V)


def test_fdr_bh_is_the_project_rule():
    from gpzoo_amd.utilities import fdr_bh
    p = np.random.default_rng(3).random(40) ** 2
    p[[5, 14, 23, 32]] = 0.005
    np.testing.assert_array_equal(Q.fdr_bh(p), fdr_bh(torch.as_tensor(p)).numpy())


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_the_planted_conditions_hold_on_the_oracle(kind, family):
    """What the GPU test asserts of the device, asserted of the fp64 oracle: the planted genes sit at the smallest attainable
    p-value, every other gene at p >= 0.02, and fdr_bh at 0.05 selects a superset of the planted genes."""
    c = R.planted_case()
    perms = Q.planted_perms()
    assert perms.shape == (199, 400) and (perms[0] == np.random.default_rng(4242).permutation(400)).all()
    planted = c["planted"]
    for mode in ("moran", "geary"):
        o = Q.planted_oracle(kind, family, mode)
        count = o["n_ge"] if mode == "moran" else o["n_le"]
        assert (count[planted] == 0).all() and (o["p"][planted] == 0.005).all()
        assert (o["p"][~planted] >= 0.02).all() and o["p"][~planted].min() >= 0.04
        assert set(o["selected"]) >= set(np.flatnonzero(planted))
        assert (o["n_ge"] + o["n_le"] >= Q.PLANTED_P).all()


def test_perm_fields_with_a_constant_gene():
    """A gene with constant residuals is not constructible on the device; its NaN handling is _perm_fields'."""
    from gpzoo_amd.ops import AutocorrPerm
    from gpzoo_amd.utilities import _perm_fields
    nan = float("nan")
    value = torch.tensor([0.3, nan], dtype=torch.float64)
    r = AutocorrPerm("moran", value, torch.tensor([2, 0], dtype=torch.int32), torch.tensor([5, 0], dtype=torch.int32),
                     torch.tensor([0.1, nan], dtype=torch.float64), torch.tensor([0.7, nan], dtype=torch.float64), None)
    P, n_ge, n_le, pg, pl, ps, mean_sim, var_sim, z_sim, pz, sims = _perm_fields(value, r, 7)
    assert P == 7 and n_ge.tolist() == [2, 0] and n_le.tolist() == [5, 0] and sims is None
    assert pg[0] == 3 / 8 and pl[0] == 6 / 8 and ps[0] == 3 / 8 and var_sim[0] == pytest.approx(0.1)
    assert all(bool(torch.isnan(t[1])) for t in (pg, pl, ps, mean_sim, var_sim, z_sim, pz))
