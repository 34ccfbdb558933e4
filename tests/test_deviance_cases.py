"""CPU: everything tests/deviance_cases.py promises the GPU tests of the Poisson deviance -- the oracle's two routes agree,
the sparse factorisation of sum mu agrees with the dense sum, every case keeps the fp32 evaluation within a third of the
tolerances, and every probe is worth at least SHARP_NEED tolerances in every output it feeds.  Tile and chunk boundaries
come from the library's host-only plan queries."""
import pytest
import torch

import deviance_cases as DC


def plans():
    from gpzoo_amd import ops
    return ops.poisson_deviance_plan, ops.poisson_deviance_sparse_plan


def all_cases():
    dplan, splan = plans()
    out = [(f"Lt{Lt}", DC.dense_case(130, 80, Lt, dplan(130, 80, Lt))) for Lt in DC.FACTOR_COUNTS]
    p = dplan(130, 80, 5)
    for e in DC.EDGE_SPOTS:
        N = DC.edge(p["spots_per_tile"], e)
        D = DC.ONE_SPOT_GENES if N == 1 else 37
        out.append((f"N{N}", DC.dense_case(N, D, 5, dplan(N, D, 5))))
    for unit, edges in ((p["genes_per_tile"], DC.EDGE_GENES), (p["genes_per_block"], DC.EDGE_BLOCKS)):
        for e in edges:
            D = DC.edge(unit, e)
            out.append((f"D{D}", DC.dense_case(70, D, 5, dplan(70, D, 5))))
    out.append(("sliced", DC.dense_case(*DC.SLICED, dplan(*DC.SLICED))))
    out += list(DC.zeros_cases().items())
    out.append(("chunks", DC.chunk_case(splan(2000, 2000, 6, 5, 1000)["gene_chunk"])))
    c, idx = DC.view_case()
    out += [("view_base", c), ("view", DC.view(c, idx))]
    return out


CASES = None


def cases():
    global CASES
    if CASES is None:
        CASES = all_cases()
    return CASES


def test_the_two_routes_of_the_oracle_agree():
    """torch.distributions.Poisson (the lgamma terms cancel) against the explicit formula, 1e-12 relative."""
    for name, c in cases():
        for flag in (True, False):
            a, b = DC.oracle(c, flag), DC.explicit(c, flag)
            for k in DC.OUTPUTS:
                scale = float(a[k].abs().max()) if a[k].numel() else 0.0
                torch.testing.assert_close(a[k], b[k], rtol=1e-12, atol=1e-12 * scale, msg=lambda m: f"{name} {k}: {m}")


def test_the_sparse_factorisation_of_sum_mu_agrees_with_the_dense_sum():
    for name, c in cases():
        for flag in (True, False):
            mu, f = DC.rate(c, flag), DC.factorised_sum_mu(c, flag)
            torch.testing.assert_close(f["per_gene"], mu.sum(1), rtol=1e-12, atol=0.0)
            torch.testing.assert_close(f["per_spot"], mu.sum(0), rtol=1e-12, atol=0.0)


def test_the_fp32_evaluation_stays_within_a_third_of_every_tolerance():
    for name, c in cases():
        for flag in (True, False):
            fig = DC.figures(DC.oracle(c, flag), DC.fp32_evaluation(c, flag))
            assert max(fig.values()) <= 1.0 / 3.0, (name, flag, fig)


def test_every_probe_is_sharp():
    seen = 0
    for name, c in cases():
        if name == "view":
            continue
        for flag in (True, False):
            s = DC.sharpness(c, flag)
            seen += len(s)
            assert all(v >= DC.SHARP_NEED for v in s), (name, flag, min(s))
    assert seen > 200


def test_one_spot_case_is_exact_and_sharp():
    c = DC.one_spot_case(DC.ONE_SPOT_GENES, 5)
    for flag in (True, False):
        ref, low = DC.oracle(c, flag), DC.fp32_evaluation(c, flag)
        assert bool((ref["null_per_gene"] == 0).all()) and bool((low["null_per_gene"] == 0).all())
        assert float(ref["null_total"]) == 0.0 and float(low["null_total"]) == 0.0
        # per_gene[d] is the unit deviance of the one element: dropped it is 0, doubled twice itself
        assert bool((ref["per_gene"] >= DC.SHARP_NEED * DC.tolerance(ref, "per_gene")).all())
        assert float(ref["per_gene"].min()) >= DC.SHARP_NEED * float(DC.tolerance(ref, "total"))
        assert float(ref["per_gene"].min()) >= DC.SHARP_NEED * float(DC.tolerance(ref, "per_spot")[0])


def test_zero_conventions():
    z = DC.zeros_cases()
    c = z["all_zero"]
    ref = DC.oracle(c)
    assert float(ref["sum_y"]) == 0.0 and float(ref["null_total"]) == 0.0 and bool((ref["null_per_gene"] == 0).all())
    assert float(ref["total"]) == pytest.approx(2.0 * float(ref["sum_mu"]), rel=1e-14)
    c = z["empty_gene_and_spot"]
    ref, mu = DC.oracle(c), DC.rate(c, True)
    assert float(ref["null_per_gene"][17]) == 0.0
    assert float(ref["per_gene"][17]) == pytest.approx(2.0 * float(mu[17].sum()), rel=1e-14)
    assert float(ref["per_spot"][66]) == pytest.approx(2.0 * float(mu[:, 66].sum()), rel=1e-14)


def test_chunk_case_rows_and_probes():
    _, splan = plans()
    chunk = splan(2000, 2000, 6, 5, 1000)["gene_chunk"]
    c = DC.chunk_case(chunk)
    nz = (c["y"] != 0).sum(1).tolist()
    assert nz[1:4] == [chunk, chunk + 1, 3 * chunk]
    probes = {(d, n) for d, n, _ in c["probes"]}
    for d, n in ((1, 0), (1, chunk - 1), (2, chunk - 1), (2, chunk), (3, chunk - 1), (3, chunk), (3, 2 * chunk - 1), (3, 2 * chunk),
                 (3, 3 * chunk - 1)):
        assert (d, n) in probes
    assert splan(c["N"], c["N"], c["D"], 5, int((c["y"] != 0).sum()))["spot_chunk"] == 0      # columns are not split


def test_view_case():
    c, idx = DC.view_case()
    spots = idx.tolist()
    assert len(spots) == 37 and 0 in spots and 129 in spots and spots != sorted(spots)
    d, n = DC.VIEW_EXCLUDED_PROBE
    assert n not in spots and (d, n) in {(a, b) for a, b, _ in c["probes"]}
    v = DC.view(c, idx)
    # were the excluded probe counted into its gene's sums, per_gene[d] would move by more than SHARP_NEED tolerances
    ref = DC.oracle(v)
    leak = float(DC.outputs_from(c["y"][d:d + 1, n:n + 1], DC.rate(c, True)[d:d + 1, n:n + 1], c["V"][n:n + 1])["total"])
    assert leak / float(DC.tolerance(ref, "per_gene")[d]) >= DC.SHARP_NEED
    assert leak / float(DC.tolerance(ref, "total")) >= DC.SHARP_NEED


def test_dense_probe_positions_follow_the_plan():
    dplan, _ = plans()
    p = dplan(*DC.SLICED)
    assert p["spot_slices"] > 1
    pos = DC.dense_positions(DC.SLICED[0], DC.SLICED[1], p)
    spots = {n for _, n in pos}
    cut = p["tiles_per_spot_slice"] * p["spots_per_tile"]
    assert {cut - 1, cut, 0, DC.SLICED[0] - 1} <= spots
    p = dplan(70, 129, 5)
    genes = {d for d, _ in DC.dense_positions(70, 129, p)}
    assert {0, 128, p["genes_per_tile"] - 1, p["genes_per_tile"], p["genes_per_block"] - 1, p["genes_per_block"]} <= genes
