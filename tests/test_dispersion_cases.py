"""CPU: the cases of tests/dispersion_cases.py are decidable and hit every branch tests/test_hip_dispersion.py is meant to
run, and their oracle is right -- against mpmath, against torch's negative-binomial density and against the moment rule."""
import math

import numpy as np
import pytest
import torch

import dispersion_cases as DC


@pytest.fixture(scope="module", autouse=True)
def _library():
    from gpzoo_amd import build
    build.build(force=False, verbose=False)


def test_rows_hit_every_branch():
    g = DC.granularity()
    assert g % 64 == 0 and DC.RTOL == 1e-11
    import gene_rank_cases as G
    assert DC.RTOL == G.DEVIANCE_RTOL
    for N in DC.NS:
        kinds = DC.row_kinds(N)
        assert len(set(kinds.values())) == len(kinds) and max(kinds.values()) < DC.D - DC.N_REST
        Y = DC.counts(N)
        nnz = (Y != 0).sum(axis=1)
        assert Y.shape == (DC.D, N) and nnz[kinds["empty"]] == 0 and nnz[kinds["one"]] == 1
        assert nnz[kinds["every"]] == N and nnz[kinds["constant"]] == N and len(set(Y[kinds["constant"]])) == 1
        for name, n in (("g-1", g - 1), ("g+0", g), ("g+1", g + 1)):
            assert (name in kinds) == (n <= N)
            if name in kinds:
                assert nnz[kinds[name]] == n
        assert 2500 <= Y[kinds["big"]].max() <= 3000 and Y[kinds["ge16"]].min() == 16 and nnz[kinds["ge16"]] == N
        assert nnz[kinds["spike"]] == 1 and Y[kinds["spike"]].max() == 20000
        H = DC.counts(N, "holes")
        assert (H[:, DC.holes(N)] == 0).all() and (DC.case_sizes(N, "holes")[DC.holes(N)] == 0).all()
        assert (DC.case_sizes(N, "holes") > 0).sum() == N - DC.holes(N).size and (DC.case_sizes(N, "totals") > 0).all()
        assert len(set(DC.case_sizes(N, "ones"))) == 1 and len(set(DC.case_sizes(N, "uniform"))) == N
    assert {"g-1", "g+0", "g+1"} <= set(DC.row_kinds(DC.NS[-1]))


@pytest.mark.parametrize("N,sizes", DC.CASES)
def test_every_boundary_decision_is_decidable(N, sizes):
    """The score changes sign at most once along the grid, and at both ends of the range |S| >= 100 x 1e-11 A, for the
    default range and, where the GPU test runs it, the narrow one: no gene is left out of any comparison of the GPU test."""
    assert (DC.sign_changes(N, sizes) <= 1).all()
    for rng in (DC.THETA_RANGE, DC.NARROW_RANGE) if (N, sizes) in DC.NARROW_CASES else (DC.THETA_RANGE,):
        o = DC.solve(N, sizes, rng)
        has = o["status"] != 4
        assert has.sum() >= (DC.D - 2 if N > 7 else 36) and o["status"][DC.row_kinds(N)["empty"]] == 4
        for end in ("lo", "hi"):
            r = np.abs(o[f"S_{end}"][has]) / o[f"A_{end}"][has]
            print(N, sizes, rng, end, "min |S| / A", r.min())
            assert (r >= 100 * DC.RTOL).all()
        inner = o["status"] == 0
        assert (o["H"][inner] < 0).all() and (o["gain"][inner] > 0).all()
        for d in np.nonzero(inner)[0]:                                # the moment start of the kernel is decidable too
            _, den, scale = DC.genes(N, sizes)[d].moment_start(rng)
            assert abs(den) >= 1e-9 * scale


def test_the_cases_reach_every_status_and_a_tight_comparison():
    tol_t = DC.plan()["tol_t"]
    assert 0 < tol_t <= 1e-9
    seen, tight = set(), {}
    for N, sizes in DC.CASES:
        o = DC.solve(N, sizes)
        seen |= set(o["status"].tolist())
        inner = o["status"] == 0
        tight[N, sizes] = int((DC.RTOL * o["A"][inner] / np.abs(o["H"][inner]) + tol_t < 1e-8).sum())
        if (N, sizes) in DC.NARROW_CASES:
            seen |= {10 + s for s in DC.solve(N, sizes, DC.NARROW_RANGE)["status"].tolist()}
    print(tight)
    assert {0, 1, 2, 4, 10, 11, 12, 14} <= seen
    assert all(v >= 12 for k, v in tight.items() if k[0] > 7), tight
    assert DC.solve(1037, "ones")["status"][DC.row_kinds(1037)["constant"]] == 1      # the same count at every spot: underdispersed


MP_GENES = [(257, "uniform", "gp-0.5-30"), (1037, "totals", "big"), (257, "ones", "spike")]


@pytest.mark.parametrize("N,sizes,kind", MP_GENES)
def test_the_oracle_holds_1e_13_against_mpmath(N, sizes, kind):
    d = DC.row_kinds(N)[kind]
    g = DC.genes(N, sizes)[d]
    o = DC.solve(N, sizes)
    thetas = [DC.THETA_RANGE[0], 1.0, 1e3, DC.THETA_RANGE[1]] + ([float(o["theta"][d])] if o["status"][d] == 0 else [])
    for th in thetas:
        S, A, _ = g.score(th)
        gain, gscale = g.gain(th)
        mS, mG, mP = DC.mp_terms(g, th)
        print(N, sizes, kind, th, "S err / A", abs(float(mS - S)) / A, "gain err / scale", abs(float(mG - gain)) / gscale)
        assert abs(float(mS - S)) <= DC.ORACLE_RTOL * A
        assert abs(float(mG - gain)) <= DC.ORACLE_RTOL * gscale
    pl, pscale = g.poisson_loglik()
    assert abs(float(mP - pl)) <= DC.ORACLE_RTOL * pscale


def test_slope_of_the_oracle_is_the_derivative_of_its_score():
    g = DC.genes(257, "uniform")[DC.row_kinds(257)["gp-2-30"]]
    for th in (0.01, 1.0, 50.0):
        e = 1e-5
        num = (g.score(th * math.exp(e))[0] - g.score(th * math.exp(-e))[0]) / (2 * e)
        assert abs(num - g.score(th)[2]) <= 1e-6 * g.score(th)[1]


@pytest.mark.parametrize("N,sizes", [(257, "uniform"), (257, "holes"), (1037, "ones")])
def test_loglik_is_the_negative_binomial_density_of_torch(N, sizes):
    """poisson_loglik + gain = sum_n log NB(y | mu, theta) (torch.distributions, fp64) at moderate theta; the zero-size
    spots of "holes" hold no counts and are left out of torch's sum."""
    Y, size = DC.case_counts(N, sizes), DC.case_sizes(N, sizes)
    for d, g in enumerate(DC.genes(N, sizes)):
        if g.sum == 0:
            continue
        keep = size > 0
        y, mu = torch.tensor(Y[d, keep], dtype=torch.float64), torch.tensor(g.mu[keep])
        pl, pscale = g.poisson_loglik()
        for th in (0.3, 5.0, 80.0):
            t = torch.tensor(th, dtype=torch.float64)
            want = torch.distributions.NegativeBinomial(total_count=t, logits=torch.log(mu) - torch.log(t)).log_prob(y)
            gain, gscale = g.gain(th)
            scale = float(want.abs().sum()) + pscale + gscale
            assert abs(pl + gain - float(want.sum())) <= 1e-11 * scale, (d, th)


def test_sign_at_the_poisson_end_is_the_moment_rule():
    """theta -> inf: S > 0 iff sum (y - mu)^2 < sum y, on the Poisson rows (and with the oracle's status at 1e6)."""
    for N, sizes in DC.CASES:
        for m in DC.MEANS:
            g = DC.genes(N, sizes)[DC.row_kinds(N)[f"poisson-{m:g}"]]
            if g.sum == 0:
                continue
            S = g.score(1e9)[0]
            under = ((g.y_all - g.mu) ** 2).sum() < g.sum
            assert (S > 0) == under, (N, sizes, m)
