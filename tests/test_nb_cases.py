"""CPU: tests/nb_cases.py covers what tests/test_hip_nb.py promises -- the lowest and the highest factor count of every
kernel instance of gpz_nb_nsf, both row-alignment paths, and every listed extent.  The instances are read from the
library's host-only plan query, not mirrored here."""
import nb_cases as NC


def plan(N, D, Lt, E):
    from gpzoo_amd import ops
    return ops.nb_nsf_plan(N, D, Lt, E)


def instances():
    """{factors_padded: (lowest Lt, highest Lt)} over every supported factor count."""
    out = {}
    for Lt in range(1, 65):
        fp = plan(64, 16, Lt, 1)["factors_padded"]
        assert fp >= Lt
        lo, hi = out.get(fp, (Lt, Lt))
        out[fp] = (min(lo, Lt), max(hi, Lt))
    return out


def test_sweep_reaches_both_ends_of_every_kernel_instance():
    inst = instances()
    assert len(inst) >= 2 and max(hi for _, hi in inst.values()) == 64
    swept = {c[2] for c in NC.SWEEP}
    for fp, (lo, hi) in inst.items():
        assert lo in swept and hi in swept, f"instance padded to {fp} factors serves {lo}..{hi}: the sweep has {sorted(swept)}"
    assert set(NC.FACTORS_REQUIRED) <= swept
    served = {plan(N, D, Lt, E)["factors_padded"] for D, N, Lt, E, _, _ in NC.SWEEP}
    assert served == set(inst)


def test_instance_ends_reach_both_ends_of_every_kernel_instance():
    """INSTANCE_ENDS runs each of the nine instances at the lowest and the highest factor count it serves, on one shape with
    aligned rows, a full and a ragged spot tile, full and a partial gene group, and one slice of either kind."""
    inst = instances()
    assert len(inst) == 9
    ends = sorted(Lt for _, _, Lt, _ in NC.INSTANCE_ENDS)
    assert ends == sorted(Lt for lo_hi in inst.values() for Lt in lo_hi) and len(ends) == 18
    assert {(D, N, E) for D, N, _, E in NC.INSTANCE_ENDS} == {(40, 68, 2)}
    for D, N, Lt, E in NC.INSTANCE_ENDS:
        p = plan(N, D, Lt, E)
        assert inst[p["factors_padded"]][0] <= Lt <= inst[p["factors_padded"]][1]
        assert p["aligned_rows"] and p["gene_slices"] == 1 and p["spot_slices"] == 1
        assert 64 < N < 128 and N % 64 and D > 32 and D % 16


def test_sweep_takes_both_alignment_paths_and_every_extent():
    aligned = {plan(N, D, Lt, E)["aligned_rows"] for D, N, Lt, E, _, _ in NC.SWEEP}
    assert aligned == {True, False}
    assert {c[0] for c in NC.SWEEP} == set(NC.GENES)
    assert {c[1] for c in NC.SWEEP} == set(NC.SPOTS)
    assert {c[3] for c in NC.SWEEP} == set(NC.SAMPLES)
    assert {c[4] for c in NC.SWEEP} == {True, False}
    assert all(isinstance(c[5], str) and c[5] for c in NC.SWEEP)
    # an unaligned case with full tiles AND a ragged last tile, an aligned one with a ragged last tile
    assert any(N % 4 and N > 64 for _, N, *_ in NC.SWEEP) and any(N % 4 == 0 and N % 64 for _, N, *_ in NC.SWEEP)


def test_inputs_reach_every_branch_of_the_count_terms():
    """Zeros, integer counts below 16 (the recurrences), counts from 16 up and the entry of 300 (lgamma / digamma)."""
    c = NC.make_inputs(130, 500, 5, 1, seed=3)
    y, th = c["y"], c["theta"]
    assert float((y == 0).float().mean()) > 0.2 and bool(((y > 0) & (y < 16)).any()) and int((y >= 16).sum()) > 1
    assert float(y[0, 0]) == 300.0 and bool((y == y.round()).all())
    assert abs(float(th.min()) - 0.3) < 1e-6 and abs(float(th.max()) - 50.0) < 1e-4
    v, g = NC.oracle(c)
    assert v == v and all(bool(torch_isfinite(t)) for t in g.values())


def torch_isfinite(t):
    import torch
    return torch.isfinite(t).all()
