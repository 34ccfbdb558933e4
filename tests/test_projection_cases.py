"""CPU: the case list of tests/test_hip_projection.py covers what it claims to (tests/projection_cases.py).  The tile size,
the column step and the N-splits come from gpz_kernel_gram_plan, a host-only query of the library: no GPU is touched."""
import os

import numpy as np
import pytest

import projection_cases as PC
import projection_oracle as PO
from conftest import GOLDEN

CASES = PC.cases()
PLANS = {c["name"]: PC.plan_of(c) for c in CASES}


def test_names_are_unique_and_every_case_has_a_reason():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    assert all(c["why"] for c in CASES)
    assert len(CASES) <= 80                      # each is one GPU launch pair of milliseconds


def test_every_kind_dimension_and_precision_is_covered():
    assert {c["kind"] for c in CASES} == set(PO.KINDS)
    assert {c["d"] for c in CASES} == {1, 2, 3, 4}
    assert {c["dtype"] for c in CASES} == {"f32", "f64"}
    # every instance of the kernel template: (kind, precision, right-hand-side block)
    inst = {(c["kind"], c["dtype"], (1 if c["per_latent"] else c["L"]) > 16) for c in CASES}
    assert inst == {(k, t, big) for k in PO.KINDS for t in ("f32", "f64") for big in (False, True)}


def test_scalar_and_per_latent_parameters_are_covered():
    R = {(c["dtype"], 1 if c["per_latent"] else c["L"]) for c in CASES}
    for t in ("f32", "f64"):
        assert (t, 1) in R and any(r > 1 for tt, r in R if tt == t)
    assert any(c["per_latent"] and c["L"] > 1 for c in CASES)            # R = 1, n = L > 1
    assert any(not c["per_latent"] and c["L"] > 1 for c in CASES)        # R = L > 1, n = 1
    assert {16, 17, 64} <= {c["L"] for c in CASES if not c["per_latent"]}  # both sides of the block switch, and the limit


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_tile_and_column_step_edges_are_covered(dtype):
    mine = [c for c in CASES if c["dtype"] == dtype]
    tile = {PLANS[c["name"]]["tile"] for c in mine}
    step = {PLANS[c["name"]]["col_step"] for c in mine}
    assert len(tile) == 1 and len(step) == 1
    tile, step = tile.pop(), step.pop()
    assert {1, tile - 1, tile, tile + 1, 2 * tile + 1} <= {c["M"] for c in mine}
    assert set(PC.EDGE_M) == {1, tile - 1, tile, tile + 1, 2 * tile + 1}   # 2 tile + 1: tile (2, 0) touches no diagonal tile
    assert {1, step - 1, step, step + 1} <= {PLANS[c["name"]]["N"] for c in mine}
    for M in PC.EDGE_M:                          # every M edge meets every N edge
        assert {1, step - 1, step, step + 1} <= {PLANS[c["name"]]["N"] for c in mine if c["M"] == M}


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_case_has_three_splits_with_a_short_last_one(dtype):
    found = []
    for c in CASES:
        p = PLANS[c["name"]]
        last = p["N"] - (p["n_splits"] - 1) * p["cols_per_split"]
        assert 0 < last <= p["cols_per_split"] and p["cols_per_split"] % p["col_step"] == 0
        if c["dtype"] == dtype and p["n_splits"] >= 3 and last < p["cols_per_split"] and last % p["col_step"]:
            found.append(c["name"])
    assert found
    assert f"splits_{dtype}" in found and f"far_tile_{dtype}" in found


def test_case_data_is_float32_representable_and_finite():
    for c in CASES[::7]:
        dat = PC.data_of(c, PLANS[c["name"]]["N"])
        assert dat["X"].shape == (PLANS[c["name"]]["N"], c["d"]) and dat["Z"].shape == (c["M"], c["d"])
        assert dat["F"].shape == (c["L"], PLANS[c["name"]]["N"])
        assert dat["sigma"].shape == ((c["L"],) if c["per_latent"] else ())
        for k in ("X", "Z", "F", "sigma", "lengthscale"):
            assert dat[k].dtype == np.float32 and np.isfinite(dat[k]).all()
        assert len({tuple(z) for z in dat["Z"]}) == c["M"]               # distinct inducing points


@pytest.mark.parametrize("name", sorted(PC.GOLDENS))
def test_fixtures_hold_the_conditions_for_a_value_comparison(name):
    """A condition, not a measurement: a fixture may be compared value by value only when its Gram matrix is well
    conditioned and the reference's own float32 run stays close to its float64 run."""
    z = np.load(os.path.join(GOLDEN, f"extra_projection_{name}.npz"))
    N, M, L, frac, cls, per_latent = PC.GOLDENS[name]
    assert float(z["cond"]) <= PC.COND_MAX == 1e4
    assert float(z["ref32_err"]) <= PC.REF32_ERR_MAX == 1e-4
    assert z["X"].shape == (N, 2) and z["Z"].shape == (M, 2) and z["F"].shape == (L, N)
    assert z["mu"].shape == z["alpha"].shape == z["b"].shape == (L, M)
    assert "G" not in z.files
    assert os.path.getsize(os.path.join(GOLDEN, f"extra_projection_{name}.npz")) < 160 * 1024
    again = PC.recipe(N, M, L, frac, int(z["data_seed"]), per_latent=per_latent)     # the stored inputs are the recipe's
    for k in ("X", "Z", "F", "sigma", "lengthscale"):
        np.testing.assert_array_equal(z[k], again[k])
