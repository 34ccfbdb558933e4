"""CPU: the cases, the classification and the bounds of tests/range_cases.py, which tests/test_hip_count_range.py relies on."""
import math

import pytest
import torch

import range_cases as R


def _regimes():
    return [R.regime_case(*k) for k in R.NB_GRID]


def test_grid_is_the_one_the_suite_promises():
    assert len(R.NB_GRID) == 20 + 15 + 3 and len(set(R.NB_GRID)) == len(R.NB_GRID)
    assert {(lv, sp) for lv, _, sp in R.POISSON_GRID} == {(lv, "narrow") for lv in R.LEVELS + (R.LARGE_LEVEL,)} | \
        {(lv, "wide") for lv in R.LEVELS if lv <= 1}
    assert not [k for k in R.NB_GRID if k[2] == "wide" and k[0] > 1]
    c = R.regime_case(1.0, 1.0, "narrow")
    assert (c["D"], c["N"], c["Lt"], c["E"]) == (33, 130, 5, 3) and c["N"] % 4 and c["D"] % 16 and c["N"] % 64
    assert c["y"].shape == (33, 130) and c["eps"].shape == (3, 5, 130) and bool((c["theta"] == 1.0).all())


def test_every_tensor_is_fp32_representable_and_counts_are_integers():
    for c in _regimes() + [R.mixed_case()]:
        for k in ("mean", "scale", "eps", "W", "V", "theta", "y", "yp"):
            assert c[k].dtype == torch.float64 and bool((c[k].float().double() == c[k]).all()), (R.case_id(c), k)
        for k in ("y", "yp"):
            assert bool((c[k] == c[k].round()).all()) and float(c[k].min()) >= 0 and float(c[k].max()) < 2 ** 24


def test_median_rate_is_the_level():
    for c in _regimes():
        med = float(R.mean_rate(c).median())
        assert c["level"] / 1.5 <= med <= 1.5 * c["level"], (R.case_id(c), med)
    c = R.mixed_case()
    med = R.mean_rate(c).median(dim=1).values
    assert bool(((med >= c["levels"] / 1.5) & (med <= 1.5 * c["levels"])).all())


def test_wide_spread_spans_decades_inside_a_tile():
    c = R.regime_case(1.0, 1.0, "wide")
    expF = torch.exp(c["mean"] + c["scale"] * c["eps"])[:, :, :64]
    assert float(expF.max() / expF.min()) >= 1e8
    mu = R.sample_rate(c)[:, :16, :64]                 # a rate is a sum over five factors: its smallest is the largest of five
    assert float(mu.max() / mu.min()) >= 1e4
    c = R.regime_case(1.0, 1.0, "narrow")
    assert float(R.sample_rate(c).max() / R.sample_rate(c).min()) <= 1e3


def test_share_of_non_zero_counts():
    for c in _regimes():
        for k in ("y", "yp"):
            share = float((c[k] > 0).double().mean())
            if c["level"] == 1e-6 and c["spread"] == "narrow":
                assert share == 0.0, (R.case_id(c), k)          # the sparse entries get an empty SparseCounts
            if c["level"] >= 1e2 and c["theta_all"] >= 1:
                assert share >= 0.9, (R.case_id(c), k, share)
    assert any(float(c["y"].max()) >= 256 for c in _regimes()) and any(float(c["yp"].max()) >= 1e4 for c in _regimes())


def test_mixed_case_structure():
    c = R.mixed_case()
    assert (c["D"], c["N"]) == (40, 130) and c["spread"] == "narrow"
    for lo in range(0, c["D"] - 15, 16):
        assert set(c["blocks"][lo:lo + 16].tolist()) == set(range(len(R.REG)))
    for d in range(c["D"]):
        assert (float(c["levels"][d]), float(c["theta"][d])) == R.REG[d % 8]
    assert torch.equal(c["V"].sort().values, torch.logspace(-2, 2, 130, dtype=torch.float64).float().double())
    assert not torch.equal(c["V"], c["V"].sort().values)
    assert [int(b) for b in c["poisson_blocks"][:8]] == [0, 1, 1, 2, 2, 2, 3, 3]


def test_whole_output_norm_would_mask_the_small_regimes():
    """The oracle's largest and smallest block max|dW| differ by at least 100x: under max|ref| over the whole output the
    rows of the small block could be wrong by their own size and pass."""
    c = R.mixed_case()
    ev = R.evaluation(c, "nb_step")
    row = ev["ref"]["dW"].abs().max(1).values
    per = [float(row[c["blocks"] == b].max()) for b in range(len(R.REG))]
    assert max(per) >= 100 * min(per), per
    whole = R.G_RTOL * ev["ref"]["dW"].abs() + R.G_ATOL * ev["ref"]["dW"].abs().max()
    assert bool((ev["bound"]["dW"] <= whole).all())
    small = c["blocks"] == per.index(min(per))
    assert float((ev["bound"]["dW"][small] / whole[small]).max()) <= 0.011


def test_theta_cancel_on_a_case_written_out():
    """C_d is the sum of the absolute values of dtheta's summands, whose plain sum is the oracle's dtheta: D = 3, N = 4."""
    f = lambda *rows: torch.tensor(rows, dtype=torch.float64)   # noqa: E731
    c = dict(mean=f([0.1, -0.2, 0.3, 0.0], [0.5, 0.25, -0.5, 0.125]), scale=f([0.5, 0.25, 0.75, 0.5], [0.25, 0.5, 0.5, 1.0]),
             eps=torch.stack([f([1.0, -1.0, 0.5, 0.0], [0.0, 2.0, -0.5, 1.0]), f([-0.5, 0.25, 0.0, 1.5], [1.0, 0.0, -2.0, 0.5])]),
             W=f([0.5, 1.0], [2.0, 0.25], [0.125, 0.0625]), V=f(1.0, 0.5, 2.0, 1.5), theta=f(0.5, 4.0, 1000.0),
             y=f([0.0, 3.0, 1.0, 0.0], [7.0, 0.0, 2.0, 40.0], [0.0, 0.0, 1.0, 0.0]))
    dig = lambda x: float(torch.digamma(torch.tensor(x, dtype=torch.float64)))   # noqa: E731
    plain, absolute = [0.0] * 3, [0.0] * 3
    for d in range(3):
        th = float(c["theta"][d])
        for n in range(4):
            y = float(c["y"][d, n])
            terms = [dig(y + th) - dig(th)]
            for e in range(2):
                mu = float(c["V"][n]) * sum(float(c["W"][d, l]) * math.exp(float(c["mean"][l, n]) + float(c["scale"][l, n]) *
                                                                          float(c["eps"][e, l, n])) for l in range(2))
                terms += [-math.log1p(mu / th) / 2, (mu - y) / (mu + th) / 2]
            plain[d] += sum(terms)
            absolute[d] += sum(abs(t) for t in terms)
    import nb_cases as NB
    _, g = NB.oracle({k: v.clone() for k, v in c.items()}, with_lgamma=False)
    torch.testing.assert_close(g["theta"], torch.tensor(plain, dtype=torch.float64), rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(R.theta_cancel(c), torch.tensor(absolute, dtype=torch.float64), rtol=1e-12, atol=0)
    assert bool((R.theta_cancel(c) >= g["theta"].abs()).all())


def test_theta_bound_generalises_the_poisson_limit_bound():
    """At theta = 1e4 C_d is at least the sum_n |psi(y + theta) - psi(theta)| of test_near_poisson_limit and at most a few
    times it (the sample-dependent summands cancel against it), while |dtheta| itself is orders of magnitude smaller."""
    c = R.regime_case(1.0, 1e4, "narrow")
    th = c["theta"][:, None]
    psi = (torch.digamma(c["y"] + th) - torch.digamma(th)).abs().sum(1)
    C = R.theta_cancel(c)
    assert bool((C >= psi).all()) and bool((C <= 4 * psi + 1e-300).all())
    assert float((R.evaluation(c, "nb_step")["ref"]["dtheta"].abs() / C).max()) < 1e-2


def test_value_bound_with_the_lgamma_term():
    c = R.regime_case(1e4, 1e2, "narrow")
    for fam, y in (("nb_step", c["y"]), ("poisson_step", c["yp"])):
        ev = R.evaluation(c, fam)
        lg = float(torch.lgamma(y + 1).sum())
        assert float(ev["ref"]["ll_lgamma"]) == pytest.approx(float(ev["ref"]["ll"]) - lg, rel=1e-14)
        assert float(ev["bound"]["ll_lgamma"]) == pytest.approx(R.LL_REL * (abs(float(ev["ref"]["ll"])) + lg) + R.LL_ABS, rel=1e-14)
        assert lg > 10 * abs(float(ev["ref"]["ll_lgamma"]))          # the two parts cancel at large counts


def test_bounds_are_the_existing_ones_in_a_regime_case():
    import deviance_cases as DC
    import nb_deviance_cases as NDC
    import poisson_cases as PC
    import sparse_nb_cases as SN
    c = R.regime_case(1.0, 1e2, "narrow")
    ev = R.evaluation(c, "nb_step")
    for k in R.STEP_GRADS:
        assert torch.equal(ev["bound"][k], SN.tolerance({k[1:]: ev["ref"][k]}, k[1:]))
    assert float(ev["bound"]["ll"]) == SN.ll_tolerance(float(ev["ref"]["ll"]))
    ev = R.evaluation(c, "poisson_step")
    ref = PC.reference(R._as_poisson(c), False)
    for k in ("ll",) + R.STEP_GRADS:
        assert torch.equal(ev["bound"][k], PC.tolerance(ref, k))
    for fam, mod in (("poisson_deviance", DC), ("nb_deviance", NDC)):
        ev = R.evaluation(c, fam)
        for k in R.OUTPUTS[fam]:
            assert torch.equal(ev["bound"][k], mod.tolerance(ev["ref"], k))


def test_mixed_bounds_are_blockwise_for_the_per_gene_outputs_only():
    c = R.mixed_case()
    for fam in R.FAMILIES:
        ev = R.evaluation(c, fam)
        blocks = c["poisson_blocks"] if fam.startswith("poisson") else c["blocks"]
        for k in R.OUTPUTS[fam]:
            ref, b = ev["ref"][k], ev["bound"][k]
            if k == "dtheta":
                assert torch.equal(b, R.G_RTOL * ref.abs() + R.G_ATOL * R.theta_cancel(c))
            elif k in R.PER_GENE:
                for blk in blocks.unique():
                    m = blocks == blk
                    assert torch.equal(b[m], R.G_RTOL * ref[m].abs() + R.G_ATOL * ref[m].abs().max())
            elif ref.dim() > 0 and k not in ("ll", "ll_lgamma"):
                assert torch.equal(b, R.G_RTOL * ref.abs() + R.G_ATOL * ref.abs().max())
    # a gene without counts: the null deviance and its bound are 0, and only an exact 0 passes
    ev = R.evaluation(c, "nb_deviance")
    empty = c["y"].sum(1) == 0
    assert bool(empty.any()) and bool((ev["ref"]["null_per_gene"][empty] == 0).all())
    got = ev["ref"]["null_per_gene"].clone()
    assert R.figure(got, ev["ref"]["null_per_gene"], ev["bound"]["null_per_gene"]) == 0.0
    got[empty] = 1e-30
    assert R.figure(got, ev["ref"]["null_per_gene"], ev["bound"]["null_per_gene"]) == float("inf")


def test_figure_flags_values_that_are_not_finite():
    ref, bound = torch.ones(3, dtype=torch.float64), torch.full((3,), 0.5, dtype=torch.float64)
    assert R.figure(torch.tensor([1.0, 1.25, 1.0]), ref, bound) == 0.5
    assert R.figure(torch.tensor([1.0, float("nan"), 1.0]), ref, bound) == float("inf")


def test_classification_floor():
    """The floor is a condition on the cases: every output it names is in domain -- the plain fp32 evaluation within a third
    of the bound -- except the deviance sums listed in F32_SHORT, which stay in the floor for the kernels."""
    seen = set()
    for c in _regimes() + [R.mixed_case()]:
        for fam in R.families_of(c):
            fig = R.f32_figures(c, fam)
            print(R.case_id(c), fam, {k: f"{v:.2g}" for k, v in fig.items()})
            assert R.missed_floor(c, fam) == [], (R.case_id(c), fam, fig)
            short = R.F32_SHORT.get((fam, R.case_id(c)), ())
            assert set(short) <= set(R.floor(c, fam))
            seen |= {(fam, R.case_id(c))} if short else set()
    assert seen == set(R.F32_SHORT)


def test_floor_is_the_stated_one():
    full = lambda c, fam: set(R.floor(c, fam)) == set(R.OUTPUTS[fam])   # noqa: E731
    for c in _regimes():
        lv, th, wide = c["level"], c["theta_all"], c["spread"] == "wide"
        for fam in R.families_of(c):
            if fam.startswith("poisson"):
                assert full(c, fam)
        assert {"ll", "ll_lgamma", "dtheta"} <= set(R.floor(c, "nb_step"))
        assert full(c, "nb_step") == (lv / th <= 100 * (1 + 1e-9))
        want = (not wide and lv <= 1) or (wide and lv <= 1 and th >= 1) or (not wide and lv == 1e2 and th >= 1)
        assert full(c, "nb_deviance") == want and (want or R.floor(c, "nb_deviance") == ())
    assert all(full(R.mixed_case(), fam) for fam in R.FAMILIES)


def test_allowed_is_the_bound_in_the_floor_and_four_times_the_fp32_error_outside():
    c = R.regime_case(1e4, 1e6, "narrow")
    ev, dom = R.evaluation(c, "nb_deviance"), R.in_domain(c, "nb_deviance")
    assert not dom["total"] and R.floor(c, "nb_deviance") == ()
    a = R.allowed(c, "nb_deviance", "total")
    assert float(a) == max(float(ev["bound"]["total"]), 4 * abs(float(ev["f32"]["total"] - ev["ref"]["total"])))
    assert torch.equal(R.allowed(c, "nb_deviance", "sum_y"), ev["bound"]["sum_y"])
    c = R.regime_case(1e4, 1e2, "narrow")                                # F32_SHORT: out of domain, but of the floor
    assert not R.in_domain(c, "poisson_deviance")["total"]
    assert torch.equal(R.allowed(c, "poisson_deviance", "total"), R.evaluation(c, "poisson_deviance")["bound"]["total"])


def test_ids_name_the_cases():
    assert len(set(R.NB_IDS)) == len(R.NB_IDS) == len(R.NB_GRID) + 1 and set(R.POISSON_IDS) <= set(R.NB_IDS)
    for cid in R.NB_IDS:
        assert R.case_id(R.lookup(cid)) == cid
    assert all(R.FAMILIES == R.families_of(R.lookup(cid)) for cid in R.POISSON_IDS)
