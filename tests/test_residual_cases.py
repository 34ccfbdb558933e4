"""CPU: everything tests/residual_cases.py gives the GPU tests -- the table reaches every branch it names, the oracle agrees
with itself, the fp32 emulation stays within a third of the recorded tolerances, and the planted case satisfies its
conditions under the oracle."""
import numpy as np
import pytest

import residual_cases as R

NAMES = tuple(r[0] for r in R.TABLE)


def test_the_table_covers_every_branch_it_names():
    shapes = {(r[1], r[2], r[3]) for r in R.TABLE}
    for want in ((1, 7, 1), (17, 63, 3), (64, 64, 4), (65, 65, 5), (130, 130, 8), (33, 257, 9), (130, 257, 20), (64, 130, 33),
                 (65, 64, 64)):
        assert want in shapes
    assert len(set(NAMES)) == len(NAMES) and all(r[4] for r in R.TABLE)
    # every k-step instance of the tile pass: k-steps of 4 factors, the instances 1..10, 12, 14, 16
    def ksteps(Lt):
        k = (Lt + 3) // 4
        return k if k <= 10 else 12 if k <= 12 else 14 if k <= 14 else 16
    assert {ksteps(r[3]) for r in R.TABLE} == set(R.ALL_K_STEPS)
    assert all(R.K_STEPS[r[3]] == ksteps(r[3]) for r in R.TABLE)
    from gpzoo_amd import ops
    assert all(ops.residual_autocorr_plan(r[2], r[1], r[3])["factors_padded"] == 4 * ksteps(r[3]) for r in R.TABLE)
    # sizes on either side of a tile (64 spots), a wave (16 genes) and a block (64 genes); rows of y with and without 16-byte
    # alignment; more than one tile and more than one block
    B, D = {r[2] for r in R.TABLE}, {r[1] for r in R.TABLE}
    assert {63, 64, 65} <= B and any(b > 128 for b in B) and any(b % 4 for b in B) and any(b % 4 == 0 for b in B)
    assert {1, 17, 64, 65} <= D and any(d > 128 for d in D)


@pytest.mark.parametrize("name", NAMES)
def test_cases_hold_what_they_promise(name):
    c = R.make_case(name)
    D, B, Lt = c["D"], c["B"], c["Lt"]
    assert c["y"].shape == (D, B) and c["mean"].shape == c["scale"].shape == (Lt, B) and c["W"].shape == (D, Lt)
    for k in ("mean", "scale", "W", "V", "theta", "y"):
        assert np.array_equal(c[k], c[k].astype(np.float32).astype(np.float64)), k           # fp32-representable
    assert (c["y"] >= 0).all() and np.array_equal(c["y"], np.round(c["y"])) and (c["W"] > 0).all() and (c["V"] > 0).all()
    lo, hi = R.THETA_RANGE
    assert c["theta"].min() == pytest.approx(lo if D > 1 else c["theta"].min()) and c["theta"].max() <= hi * 1.0001
    if D >= 17:
        assert c["theta"].min() < 0.06 and c["theta"].max() > 0.9e7 and not (np.diff(c["theta"]) > 0).all()
    # the probes: the corners and the edges of tiles, waves and blocks; a large count or a zero beside a large rate
    mu, pos = R.rate(c), {(g, s) for g, s, _ in c["probes"]}
    assert {(0, 0), (0, B - 1), (D - 1, 0), (D - 1, B - 1)} <= pos
    for g in (15, 16, 63, 64):
        for s in (63, 64):
            assert ((g, s) in pos) == (g < D and s < B)
    big = [(g, s) for g, s, cnt in c["probes"] if cnt > 0]
    zero = [(g, s) for g, s, cnt in c["probes"] if cnt == 0]
    assert big and all(c["y"][g, s] >= R.BIG_COUNT and c["y"][g, s] > 20 * mu[g, s] for g, s in big)
    if len(c["probes"]) > 1:
        assert zero and all(c["y"][g, s] == 0 and mu[g, s] > 3.0 for g, s in zero)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_agrees_with_itself(name):
    c = R.make_case(name)
    y, mu, th = c["y"], R.rate(c), c["theta"]
    # Pearson residuals of NB at theta = 1e7 are the Poisson ones to 1e-6 relative.  The two differ by the factor
    # 1 / sqrt(1 + mu / theta) = 1 - mu / (2 theta) + ..., so the statement is one about rates up to 2e-6 theta = 20: it is
    # asserted at every such element (a fifth of each case or more), and the factor itself at every element, the probes' large rates included
    p, nb = R.residuals(y, mu, "pearson"), R.residuals(y, mu, "pearson", np.full(c["D"], 1e7))
    small = mu <= 20.0
    assert small.mean() > 0.2 and (np.abs(nb - p)[small] <= 1e-6 * np.abs(p)[small]).all()
    assert np.allclose(nb * np.sqrt(1.0 + mu / 1e7), p, rtol=1e-13, atol=0.0)
    # d >= 0 everywhere, in both families; 2 mu at y = 0
    dp, dn = R.unit_deviance(y, mu), R.unit_deviance(y, mu, th)
    assert (dp >= 0).all() and (dn >= 0).all()
    assert np.allclose(dp[y == 0], 2.0 * mu[y == 0], rtol=1e-14)
    # the two NB deviance forms agree: the split form rounds (y + theta) / (mu + theta) next to 1, an absolute error of a few
    # 2^-53 in its logarithm that theta multiplies, and loses y A against theta B; nothing else separates them
    split = R.unit_deviance_nb_split(y, mu, th)
    assert (np.abs(split - dn) <= 1e-12 * (1.0 + np.abs(dn) + y) + 16.0 * 2.0 ** -53 * (th[:, None] + y)).all()
    # the deviance residual has the sign of y - mu and the NB one tends to the Poisson one
    r = R.residuals(y, mu, "deviance", th)
    assert (np.sign(r) == np.sign(y - mu)).all()
    far = R.residuals(y, mu, "deviance", np.full(c["D"], 1e9))
    assert np.allclose(far, R.residuals(y, mu, "deviance"), rtol=1e-5, atol=1e-7)


def test_morans_i_oracle_is_the_double_sum():
    rng = np.random.default_rng(0)
    Rm, nbr = rng.standard_normal((3, 50)), R.random_table(50, 4)
    I, mean, var = R.morans_i(Rm, nbr)
    for g in range(3):
        z = Rm[g] - Rm[g].mean()
        num = sum(z[n] * sum(z[j] for j in nbr[n]) / 4.0 for n in range(50))
        assert I[g] == pytest.approx(num / (z * z).sum(), rel=1e-12) and var[g] == pytest.approx((z * z).mean(), rel=1e-12)
    assert np.allclose(mean, Rm.mean(axis=1))
    assert (nbr != np.arange(50)[:, None]).all() and all(len(set(row)) == 4 for row in nbr.tolist())
    X = rng.random((40, 2))
    knn = R.knn_table(X, 3)
    d = ((X[:, None] - X[None]) ** 2).sum(-1)
    assert all(set(knn[i]) == set(np.argsort(d[i] + 1e9 * (np.arange(40) == i))[:3]) for i in range(40))


@pytest.mark.parametrize("name", NAMES)
def test_emulation_stays_within_a_third_of_the_tolerances(name):
    c = R.make_case(name)
    for kind in R.KINDS:
        for family in R.FAMILIES:
            ref, got = R.oracle_residuals(c, kind, family), R.emulate_residuals(c, kind, family)
            rel, ab = R.residual_errors(ref, got)
            assert 3.0 * rel <= R.RTOL and 3.0 * ab <= R.ATOL, (kind, family, rel, ab)
            assert R.residual_figure(ref, got) <= 1.0 / 3.0
    assert 3.0 * R.i_error(c, R.case_table(c)) <= R.I_ATOL


def test_planted_case_satisfies_its_conditions_under_the_oracle():
    c = R.planted_case()
    assert c["y"].shape == (40, 400) and c["planted"].sum() == 4 and c["nbr"].shape == (400, 6)
    assert (c["nbr"] != np.arange(400)[:, None]).all()
    gx = np.round(c["X"][:, 0] - 0.025)
    assert set(gx.tolist()) == set(range(20))                                # a 20 x 20 grid
    for kind in R.KINDS:
        for family in R.FAMILIES:
            I = R.morans_i(R.oracle_residuals(c, kind, family), c["nbr"])[0]
            z = R.moran_z(I, c["nbr"])
            assert R.planted_conditions(z, c["planted"]) == (True, True, True), (kind, family, z)
