"""CPU: everything tests/nb_deviance_cases.py promises the GPU tests of the NB deviance -- the oracle agrees with the
written-out formulas, the sparse decomposition (zero part plus stored-entry corrections) reproduces the dense sums, every
case keeps the fp32 evaluation within a third of the tolerances under both values of lognormal_mean, every probe is worth
at least SHARP_NEED tolerances in every output it feeds, and at theta = 1e7 the NB outputs are the Poisson ones to within
a third of a tolerance.  Tile and chunk boundaries come from the library's host-only plan queries."""
import torch

import deviance_cases as DC
import nb_deviance_cases as NC


def plans():
    from gpzoo_amd import ops
    return ops.nb_deviance_plan, ops.nb_deviance_sparse_plan


def all_cases():
    dplan, splan = plans()
    out = [(f"Lt{Lt}", NC.dense_case(130, 80, Lt, dplan(130, 80, Lt))) for Lt in DC.FACTOR_COUNTS]
    p = dplan(130, 80, 5)
    for e in DC.EDGE_SPOTS:
        N = DC.edge(p["spots_per_tile"], e)
        D = DC.ONE_SPOT_GENES if N == 1 else 37
        out.append((f"N{N}", NC.dense_case(N, D, 5, dplan(N, D, 5))))
    for unit, edges in ((p["genes_per_tile"], DC.EDGE_GENES), (p["genes_per_block"], DC.EDGE_BLOCKS)):
        for e in edges:
            D = DC.edge(unit, e)
            out.append((f"D{D}", NC.dense_case(70, D, 5, dplan(70, D, 5))))
    out.append(("sliced", NC.dense_case(*DC.SLICED, dplan(*DC.SLICED))))
    out += list(NC.zeros_cases().items())
    out.append(("chunks", NC.chunk_case(splan(2000, 2000, 6, 5, 1000)["gene_chunk"])))
    c, idx = NC.view_case()
    out += [("view_base", c), ("view", NC.view(c, idx))]
    pm = dplan(*NC.MID)
    pos = DC.dense_positions(NC.MID[0], NC.MID[1], pm)
    out.append(("theta-small", NC.make_probe_case(*NC.MID, pos, seed=12, theta=NC.THETA_SMALL)))
    out.append(("theta-large", NC.make_probe_case(*NC.MID, pos, seed=13, theta=NC.THETA_LARGE)))
    out.append(("theta-mixed", NC.make_probe_case(*NC.MID, pos, seed=14, theta=NC.mixed_theta(NC.MID[1], pm["genes_per_tile"]))))
    out.append(("same", NC.make_probe_case(*NC.MID, pos, seed=9, density=0.2)))
    out.append(("sliced-large", NC.dense_case(*DC.SLICED, dplan(*DC.SLICED), theta=NC.THETA_LARGE)))
    out.append(("chunks-large", NC.chunk_case(splan(2000, 2000, 6, 5, 1000)["gene_chunk"], theta=NC.THETA_LARGE)))
    out.append(("limit", NC.limit_case()))
    return out


CASES = None


def cases():
    global CASES
    if CASES is None:
        CASES = all_cases()
    return CASES


def _lgamma_rounding(c):
    """What fp64 itself loses in lgamma(y + theta) - lgamma(theta), summed over the case: both routes take that difference,
    in different orders, and each lgamma is rounded at 2^-52 of its own size -- 1.5e8 at theta = 1e7.  Nothing at the
    default theta (<= 50), where the bound is the plain 1e-12."""
    th = float(c["theta"].max())
    if th <= NC.THETA_RANGE[1]:
        return 0.0
    return c["y"].numel() * 2.0 ** -52 * 2.0 * float(torch.lgamma(c["theta"].max() + c["y"].max()))


def _close(a, b, names, what, extra=0.0):
    for k in names:
        scale = float(a[k].abs().max()) if a[k].numel() else 0.0
        torch.testing.assert_close(a[k], b[k], rtol=1e-12, atol=1e-12 * scale + extra, msg=lambda m: f"{what} {k}: {m}")


def test_the_plans_report_the_units_of_the_poisson_entry():
    from gpzoo_amd import ops
    dplan, splan = plans()
    for shape in ((130, 80, 5), DC.SLICED, (7000, 17702, 20)):
        a, b = dplan(*shape), ops.poisson_deviance_plan(*shape)
        assert {k: v for k, v in a.items() if k != "workspace_bytes"} == {k: v for k, v in b.items() if k != "workspace_bytes"}
    assert splan(2000, 2000, 6, 5, 1000)["gene_chunk"] == ops.poisson_deviance_sparse_plan(2000, 2000, 6, 5, 1000)["gene_chunk"]


def test_the_oracle_agrees_with_the_written_out_formulas():
    for name, c in cases():
        for flag in (True, False):
            _close(NC.oracle(c, flag), NC.explicit(c, flag), NC.OUTPUTS, f"{name} {flag}", _lgamma_rounding(c))


def test_the_sparse_decomposition_reproduces_the_dense_oracle():
    seen_unsorted = False
    for name, c in cases():
        for flag in (True, False):
            _close(NC.oracle(c, flag), NC.sparse_decomposition(c, flag), NC.OUTPUTS, f"{name} {flag}", _lgamma_rounding(c))
        seen_unsorted |= name == "view"
    c, idx = NC.view_case()
    assert seen_unsorted and bool((idx[1:] < idx[:-1]).any())


def test_the_fp32_evaluation_stays_within_a_third_of_every_tolerance():
    for name, c in cases():
        for flag in (True, False):
            fig = NC.figures(NC.oracle(c, flag), NC.fp32_evaluation(c, flag))
            assert max(fig.values()) <= 1.0 / 3.0, (name, flag, fig)


def test_every_probe_is_sharp():
    """In every output a probe feeds; see nb_deviance_cases.fully_probed for the four outputs that only the cases with one
    large theta for every gene can probe, and for why."""
    seen, full = 0, set()
    for name, c in cases():
        if name == "view":
            continue
        for flag in (True, False):
            s = NC.sharpness(c, flag)
            seen += len(s)
            assert all(v >= NC.SHARP_NEED for v in s), (name, flag, min(s))
        if NC.fully_probed(c) and c["probes"]:
            full.add(name)
    assert seen > 200 and full == {"theta-large", "sliced-large", "chunks-large"}


def test_theta_is_log_spaced_and_representable():
    th = NC.default_theta(80)
    assert float(th[0]) == float(torch.tensor(0.3).float()) and float(th[-1]) == float(torch.tensor(50.0).float())
    assert torch.equal(th, th.float().double()) and bool((th[1:] > th[:-1]).all())
    m = NC.mixed_theta(80, 16)
    assert float(m[:16].min()) < 0.31 and float(m[:16].max()) > 9e5 and torch.equal(m[:16], m[16:32])


def test_zero_conventions():
    z = NC.zeros_cases()
    c = z["all_zero"]
    ref, mu, th = NC.oracle(c), DC.rate(c, True), c["theta"][:, None]
    assert float(ref["sum_y"]) == 0.0 and float(ref["null_total"]) == 0.0 and bool((ref["null_per_gene"] == 0).all())
    zz = th * torch.log1p(mu / th)
    torch.testing.assert_close(ref["total"], 2.0 * zz.sum(), rtol=1e-12, atol=0.0)
    torch.testing.assert_close(ref["loglik"], -zz.sum(), rtol=1e-12, atol=0.0)
    torch.testing.assert_close(ref["poisson_loglik"], -mu.sum(), rtol=1e-12, atol=0.0)
    c = z["empty_gene_and_spot"]
    ref = NC.oracle(c)
    assert float(ref["null_per_gene"][17]) == 0.0 and bool((c["y"][17] == 0).all()) and bool((c["y"][:, 66] == 0).all())


def test_one_spot_null_deviance_is_exactly_zero():
    c = NC.dense_case(1, DC.ONE_SPOT_GENES, 5, None)
    for flag in (True, False):
        ref, low = NC.oracle(c, flag), NC.fp32_evaluation(c, flag)
        assert bool((ref["null_per_gene"] == 0).all()) and bool((low["null_per_gene"] == 0).all())
        assert float(ref["null_total"]) == 0.0 and float(low["null_total"]) == 0.0


def test_the_poisson_limit():
    """theta = 1e7 on a probe-free case: NB total / per_gene within a third of a tolerance of the Poisson oracle, loglik
    within a third of poisson_loglik -- what makes the GPU test against ops.poisson_deviance meaningful."""
    c = NC.limit_case()
    assert not c["probes"] and bool((c["theta"] == 1e7).all())
    for flag in (True, False):
        nb, po = NC.oracle(c, flag), DC.oracle(c, flag)
        for k in ("total", "per_gene", "per_spot", "null_per_gene", "null_total", "sum_y", "sum_mu"):
            err, tol = (nb[k] - po[k]).abs(), DC.tolerance(po, k)
            assert float((err / tol).max()) <= 1.0 / 3.0, (k, flag, float((err / tol).max()))
        for a, b in (("loglik", "poisson_loglik"), ("loglik_per_gene", "poisson_loglik_per_gene")):
            err, tol = (nb[a] - nb[b]).abs(), NC.tolerance(nb, b)
            assert float((err / tol).max()) <= 1.0 / 3.0, (a, flag, float((err / tol).max()))
