"""CPU: the table of tests/scratch_cases.py -- every entry of include/gpzoo_hip.h that takes a workspace has a row, SMALL is
one slice and LARGE at least two in every count of the plan, LARGE needs more scratch than SMALL, and every input is
finite and exactly representable in the type it is run in.  The plan and workspace queries need no device."""
import os

import pytest
import torch

import scratch_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [r.name for r in S.ROWS]


@pytest.fixture(scope="module", autouse=True)
def _library():
    from gpzoo_amd import build
    build.build(force=False, verbose=False)


def test_every_entry_that_takes_a_workspace_has_a_row():
    hdr = open(os.path.join(ROOT, "include", "gpzoo_hip.h")).read()
    want = S.header_entries_with_workspace(hdr)
    assert len(want) >= 29 and "gpz_svgp_forward" in want and "gpz_nb_deviance_sparse" in want and "gpz_counts_matmul" in want
    assert "gpz_kfill" not in want and "gpz_allreduce_sum_f64" not in want
    have = {e for r in S.ROWS for e in r.entries}
    assert not want - have, f"no row of tests/scratch_cases.py runs {sorted(want - have)}"
    import re
    declared = set(re.findall(r"\b(gpz_[a-z0-9_]+)\s*\(", hdr))
    assert have <= declared, sorted(have - declared)


# every row by name: taking one out, or renaming it, fails test_the_table_is_exactly_these_rows
ROW_NAMES = [
    "kgrad-f32", "kgrad-f64", "factor-f64", "factor-f32", "svgp_forward-path0", "svgp_forward-path1",
    "svgp_forward-path0-generate_refused", "svgp_forward-path3", "svgp_forward-path4", "svgp_forward-f32-unwhitened",
    "svgp_forward-f64-whitened", "svgp_forward-f64-unwhitened", "svgp_forward-f32-chunks", "svgp_forward-path4-chunks",
    "svgp_forward-f64-chunks", "svgp_forward-no_y-chol", "svgp_forward-retain_wt", "svgp_forward-retain_wt-chunks",
    "svgp_forward-factor_cache-f32", "svgp_forward-factor_cache-f64-unwhitened",
    "svgp_backward-classic-wide-qu-nowt-f32", "svgp_backward-classic-wide-qu-nowt-f64-unwhitened",
    "svgp_backward-classic-wide-qu-wt-f32-chunks", "svgp_backward-classic-wide-qu-wt-f64-unwhitened-chunks",
    "svgp_backward-classic-wide-all-nowt-f32-chunks", "svgp_backward-classic-wide-all-nowt-f64-unwhitened-chunks",
    "svgp_backward-classic-wide-all-wt-f32", "svgp_backward-classic-wide-all-wt-f64-unwhitened",
    "svgp_backward-classic-narrow-qu-nowt-f32", "svgp_backward-classic-narrow-qu-nowt-f64-unwhitened",
    "svgp_backward-classic-narrow-qu-wt-f32-chunks", "svgp_backward-classic-narrow-qu-wt-f64-unwhitened-chunks",
    "svgp_backward-classic-narrow-all-nowt-f32-chunks", "svgp_backward-classic-narrow-all-nowt-f64-unwhitened-chunks",
    "svgp_backward-classic-narrow-all-wt-f32", "svgp_backward-classic-narrow-all-wt-f64-unwhitened",
    "svgp_backward-algebra-wide-qu-nowt-f32", "svgp_backward-algebra-wide-qu-nowt-f64-unwhitened",
    "svgp_backward-algebra-wide-qu-wt-f32-chunks", "svgp_backward-algebra-wide-qu-wt-f64-unwhitened-chunks",
    "svgp_backward-algebra-wide-all-nowt-f32-chunks", "svgp_backward-algebra-wide-all-nowt-f64-unwhitened-chunks",
    "svgp_backward-algebra-wide-all-wt-f32", "svgp_backward-algebra-wide-all-wt-f64-unwhitened",
    "svgp_backward-algebra-narrow-qu-nowt-f32", "svgp_backward-algebra-narrow-qu-nowt-f64-unwhitened",
    "svgp_backward-algebra-narrow-qu-wt-f32-chunks", "svgp_backward-algebra-narrow-qu-wt-f64-unwhitened-chunks",
    "svgp_backward-algebra-narrow-all-nowt-f32-chunks", "svgp_backward-algebra-narrow-all-nowt-f64-unwhitened-chunks",
    "svgp_backward-algebra-narrow-all-wt-f32", "svgp_backward-algebra-narrow-all-wt-f64-unwhitened",
    "wsvgp_precomputed-f32", "wsvgp_precomputed-f64", "vnngp-f32-plain", "vnngp-f32-state-grads-order",
    "vnngp-f64-plain", "vnngp-f64-state-grads-order", "spatial_knn-order", "spatial_knn-no_order", "morans_i",
    "knn_mean", "kmeans_seed", "kmeans_lloyd", "kmeans_assign", "kernel_gram-R3", "kernel_gram-per_latent", "nmf_kl-f32",
    "nmf_kl-f64", "poisson_nsf_sparse-full-lgamma", "poisson_nsf_sparse-batch-no_lgamma", "nb_nsf_sparse-full-lgamma",
    "nb_nsf_sparse-batch-no_lgamma", "nb_nsf_sparse-full-lgamma-E33", "poisson_nsf", "poisson_nsf-gene_slices",
    "nb_nsf-lgamma", "nb_nsf-no_lgamma", "nb_nsf-lgamma-E33", "poisson_deviance", "poisson_deviance_sparse",
    "nb_deviance", "nb_deviance_sparse", "nmf_kl_sparse-f32", "nmf_kl_sparse-f64", "counts_matmul-plain",
    "counts_matmul-transpose",
]


def test_the_table_is_exactly_these_rows():
    assert IDS == ROW_NAMES, (sorted(set(ROW_NAMES) - set(IDS)), sorted(set(IDS) - set(ROW_NAMES)))
    assert all(r.check is not None for r in S.ROWS)
    bwd = [n for n in IDS if n.startswith("svgp_backward-")]
    assert len(bwd) == 32
    for a, b in (("classic", "algebra"), ("narrow", "wide"), ("-all-", "-qu-"), ("-wt-", "-nowt-"), ("f32", "f64")):
        assert any(a in n for n in bwd) and any(b in n for n in bwd)


@pytest.mark.parametrize("name", IDS)
def test_small_is_one_slice_and_large_at_least_two(name):
    r = S.row(name)
    if r.slices is not None:
        small, large = r.slices("small"), r.slices("large")
        print(name, "small", small, "large", large)
        assert small and set(small) == set(large)
        assert all(v == 1 for v in small.values()), small
        assert all(v >= 2 for v in large.values()), large
    if r.bytes is not None:
        nb_small, nb_large = int(r.bytes("small")), int(r.bytes("large"))
        print(name, "workspace bytes", nb_small, nb_large)
        assert 0 < nb_small < nb_large


@pytest.mark.parametrize("name", [n for n in IDS if n.startswith("svgp_forward-path")])
def test_forward_rows_take_the_path_they_name(name):
    want = int(name.split("path")[1][0])
    _, dt, wh, sh, kw, path = next(v for v in S.FORWARD_VARIANTS if "svgp_forward-" + v[0] == name)
    assert path == want
    for which in S.WHICH:
        assert S.svgp_forward_path(S.row(name).inputs(which), wh, **kw) == want, which


def _exact(t: torch.Tensor, dtype) -> bool:
    return bool(torch.equal(t.to(dtype).to(t.dtype), t))


@pytest.mark.parametrize("name", IDS)
def test_inputs_are_finite_and_exact_in_the_run_dtype(name):
    r = S.row(name)
    for which in S.WHICH:
        c = r.inputs(which)
        seen = 0
        for k, v in c.items():
            if not isinstance(v, torch.Tensor) or not v.is_floating_point():
                continue
            seen += 1
            assert bool(torch.isfinite(v).all()), (which, k)
            if v.dtype == torch.float64 and k in ("u", "C0", "Qd", "Qn", "g_kl"):
                continue                      # fp64 arguments of the entry whatever the row's dtype
            assert _exact(v, r.dtype), (which, k)
        assert seen >= 1


def test_extents_are_off_their_tile_multiples():
    """SMALL of the rows the issue names: N no multiple of 64 nor of 4, D none of 16, M none of 128, Lt none of 4 where
    the factor count is free (the Poisson and NB steps keep the notebooks' Lt = 20: their tail instance is KS = 5)."""
    for shapes in (S.NB_SHAPES, S.SP_SHAPES):
        for N, D, Lt, E in shapes.values():
            assert N % 64 and N % 4 and D % 16
    for N, D, Lt in S.DEV_SHAPES.values():
        assert N % 64 and D % 16 and Lt % 4
    for sh in (S.SVGP_TILE, S.SVGP_PAD, S.VNN_SHAPES):
        for N, M, L in sh.values():
            assert N % 128 and (M % 128 or sh is S.SVGP_TILE)
    for M, N in S.FACTOR_SHAPES.values():
        assert M % 128 and N % 128


def _finite(x) -> bool:
    if isinstance(x, dict):
        return all(_finite(v) for v in x.values())
    if isinstance(x, (tuple, list)):
        return all(_finite(v) for v in x)
    if isinstance(x, torch.Tensor):
        return bool(torch.isfinite(x.double()).all()) if x.is_floating_point() else True
    return x == x if isinstance(x, float) else True


REFERENCES = {
    "poisson_nsf": lambda c: S.PC.reference(c, True),
    "poisson_nsf-gene_slices": lambda c: S.PC.reference(c, True),
    "nb_nsf-lgamma": lambda c: S.NBC.oracle(c, True),
    "nb_nsf-lgamma-E33": lambda c: S.NBC.oracle(c, True),
    "poisson_nsf_sparse-full-lgamma": lambda c: S.SPC.reference(c, True),
    "poisson_nsf_sparse-batch-no_lgamma": lambda c: S.SPC.reference(c, False),
    "nb_nsf_sparse-full-lgamma": lambda c: S.SNC.reference(c, True),
    "nb_nsf_sparse-batch-no_lgamma": lambda c: S.SNC.reference(c, False),
    "poisson_deviance": lambda c: S.DC.oracle(c, True),
    "nb_deviance": lambda c: S.NDC.oracle(c, True),
    "kgrad-f32": lambda c: S.EC.kernel_grads(c, c["Kbar"]),
    "wsvgp_precomputed-f32": lambda c: {k: v for k, v in S.EC.precomputed_ref(c).items()},
    "factor-f64": lambda c: torch.linalg.cholesky(c["A"].double()),
    "factor-f32": lambda c: torch.linalg.cholesky(c["A"].double()),
    "svgp_forward-path1": lambda c: _forward_reference(c, True),
    "svgp_forward-path4": lambda c: _forward_reference(c, True),
    "svgp_forward-f64-unwhitened": lambda c: _forward_reference(c, False),
    "svgp_backward-classic-wide-all-wt-f32": lambda c: _backward_reference(c, True),
    "svgp_backward-classic-wide-all-wt-f64-unwhitened": lambda c: _backward_reference(c, False),
}


def _forward_reference(c, whitened):
    from oracle import svgp_oracle as O
    d = {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in c.items()}
    return O.elbo_eval(c["kind"], whitened, d["X"], d["y"], d["Z"], d["sigma"], d["lengthscale"], d["mu"], d["Lu_raw"], c["jitter"],
                       c["noise_sd"])


def _backward_reference(c, whitened):
    import backward_forms_cases as BC
    return {k: v for k, v in BC.oracle_grads(c, whitened, "dense").items() if k != "clamped"}


@pytest.mark.parametrize("name", list(REFERENCES))
def test_references_are_finite_on_the_cpu(name):
    """The oracles the GPU test compares with, evaluated here once per shared case (cached in the case modules): one row of
    every family of inputs -- the other rows of a family share its cases."""
    assert name in IDS
    for which in S.WHICH:
        assert _finite(REFERENCES[name](S.row(name).inputs(which))), (name, which)
