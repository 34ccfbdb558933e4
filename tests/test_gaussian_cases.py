"""CPU: the case list of tests/gaussian_cases.py -- it visits every kernel instance gpz_gaussian_fa_plan reports, both
alignment paths, one and several slices of both passes and every listed extent; the fp64 oracle is finite on it; and
torch's own fp32 evaluation of the closed form lies inside the tolerances the GPU test applies to the fused step."""
import pytest
import torch

import gaussian_cases as GC


@pytest.fixture(scope="module", autouse=True)
def _library():
    from gpzoo_amd import build
    build.build(force=False, verbose=False)


def plans():
    from gpzoo_amd import ops
    return [ops.gaussian_fa_plan(N, D, Lt) for D, N, Lt, _ in GC.SWEEP]


def test_sweep_visits_every_instance_path_and_extent():
    from gpzoo_amd import ops
    assert {D for D, _, _, _ in GC.SWEEP} >= set(GC.GENES)
    assert {N for _, N, _, _ in GC.SWEEP} >= set(GC.SPOTS)
    assert {Lt for _, _, Lt, _ in GC.SWEEP} >= set(GC.FACTORS_REQUIRED)
    # the required factor counts are the lowest and highest of every instance the library has
    padded = [ops.gaussian_fa_plan(64, 16, Lt)["factors_padded"] for Lt in range(1, 65)]
    edges = {Lt for Lt in range(1, 65) if Lt == 1 or Lt == 64 or padded[Lt - 1] != padded[Lt - 2] or padded[Lt] != padded[Lt - 1]}
    assert edges == set(GC.FACTORS_REQUIRED), sorted(edges ^ set(GC.FACTORS_REQUIRED))
    assert len(set(padded)) == 13
    pl = plans()
    assert {p["factors_padded"] for p in pl} == set(padded)
    assert {p["aligned_rows"] for p in pl} == {True, False}
    for key in ("gene_slices", "spot_slices"):
        assert any(p[key] == 1 for p in pl) and any(p[key] >= 2 for p in pl), key
    # several slices with aligned and with unaligned rows
    assert {p["aligned_rows"] for p in pl if p["gene_slices"] >= 2 and p["spot_slices"] >= 2} == {True, False}
    assert all(p["partials_bytes"] > 0 for p in pl)


@pytest.mark.parametrize("i", range(len(GC.SWEEP)))
def test_oracle_is_finite_and_fp32_torch_is_inside_the_tolerances(i):
    from gpzoo_amd import ops
    D, N, Lt, why = GC.SWEEP[i]
    c, want = GC.case(i)
    # the shape is one the entry takes, on the instance and the row path the case's note names
    p = ops.gaussian_fa_plan(N, D, Lt)
    assert Lt <= p["factors_padded"] < Lt + 8 and p["factors_padded"] % 4 == 0
    assert p["aligned_rows"] == (N % 4 == 0) and p["gene_slices"] >= 1 and p["spot_slices"] >= 1
    assert 0 < p["partials_bytes"] and (D * N < 4096 or p["partials_bytes"] < 32 * 4 * D * N)
    assert c["y"].shape == (D, N) and c["mean"].shape == (Lt, N) and float(c["y"][0, 0]) == 300.0
    assert float(c["sd"].min()) > 0
    assert want.value == want.value and abs(want.value) < float("inf")
    assert bool(torch.isfinite(want.sse).all()) and bool(torch.isfinite(want.sse_atol).all())
    assert all(bool(torch.isfinite(g).all()) for g in want.grads.values())
    val, sse, grads = GC.torch_fp32(c)
    GC.check(val, sse, grads, want, dict(D=D, N=N, Lt=Lt, why=why))
