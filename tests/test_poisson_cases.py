"""CPU: the case lists, the restated launch arithmetic, the probes and the fp64 reference of tests/poisson_cases.py are
what tests/test_hip_poisson_forms.py takes them for -- the lists reach every kernel instance, tail length and plan
branch they claim, the restated workspace size is the library's, the reference is the Poisson log-density, and every
probe count is *sharp*: setting that one entry of y to zero moves each output it feeds by at least ten times the
tolerance of the GPU comparison, so a kernel that drops or double-counts the element cannot pass."""
import pytest
import torch

import poisson_cases as PC

ALL_KS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16)
PROBE_CASES = PC.PLAN_CASES + [PC.HOST_SPLIT]


def test_factor_lists_reach_every_instance_tail_and_padded_dispatch():
    plans = {Lt: PC.plan(70, 37, Lt, 2) for _, _, Lt, _ in PC.FACTOR_SWEEP}
    assert sorted(plans) == list(range(1, 65))
    assert sorted({p["KS"] for p in plans.values()}) == list(ALL_KS)
    for KS in (1, 5, 9):      # the vector tail of pass B with every length
        assert sorted(p["tail_len"] for p in plans.values() if p["KS"] == KS) == [1, 2, 3, 4]
    assert all(p["TAIL"] == (p["KS"] in (1, 5, 9)) and (p["tail_len"] > 0) == p["TAIL"] for p in plans.values())
    assert all(plans[Lt]["LTM"] == 0 for Lt in (1, 2, 3, 4)) and plans[17]["LTM"] == 1 and plans[36]["LTM"] == 2
    assert plans[16]["LTM"] == 1 and plans[64]["LTM"] == 4 and plans[20]["tail_len"] == 4
    # a whole zero k-step: Lt 41..44 run KS = 12, Lt 49..52 run KS = 14 and Lt 57..60 run KS = 16; nothing else is padded
    assert [Lt for Lt, p in plans.items() if p["padded_ksteps"]] == [41, 42, 43, 44, 49, 50, 51, 52, 57, 58, 59, 60]
    assert {plans[Lt]["KS"] for Lt in (41, 42, 43, 44)} == {12} and {plans[Lt]["KS"] for Lt in (49, 50, 51, 52)} == {14}
    assert {plans[Lt]["KS"] for Lt in (57, 58, 59, 60)} == {16} and max(p["padded_ksteps"] for p in plans.values()) == 1
    assert all(p["lds_optin"] == (Lt >= 17) for Lt, p in plans.items())
    # the interior path at (128, 64): the smallest and the largest factor count of each instance
    ends = {}
    for N, D, Lt, E in PC.INSTANCE_ENDS:
        assert (N, D, E) == (128, 64, 2)
        ends.setdefault(PC.kernel_instance(Lt), []).append(Lt)
    assert ends == {1: [1, 4], 2: [5, 8], 3: [9, 12], 4: [13, 16], 5: [17, 20], 6: [21, 24], 7: [25, 28], 8: [29, 32],
                    9: [33, 36], 10: [37, 40], 12: [41, 48], 14: [49, 56], 16: [57, 64]}


def test_tile_edge_list():
    assert PC.EDGE_N == (1, 3, 4, 63, 64, 65, 66, 68, 127, 128, 129, 130, 192)
    assert PC.EDGE_D == (1, 15, 16, 17, 63, 64, 65, 149)
    assert len(PC.TILE_EDGES) == 2 * (13 + 8) and {c[3] for c in PC.TILE_EDGES} == {3}
    assert {(c[2], PC.plan(*c)["TAIL"]) for c in PC.TILE_EDGES} == {(20, True), (8, False)}
    assert {c[0] for c in PC.TILE_EDGES if c[1] == 37} == set(PC.EDGE_N)
    assert {c[1] for c in PC.TILE_EDGES if c[0] == 68} == set(PC.EDGE_D) | {37}
    # D = 149: ten 16-gene groups, so wave 0 and 1 of pass A take a second (prefetched) group and the last one is ragged
    assert PC.cdiv(149, 16) == 10 and 149 % 16 == 5


def test_plan_cases_reach_their_branches():
    p = {c: PC.plan(*c) for c in PROBE_CASES}
    assert {q["S"] for q in p.values()} == {1, 2, 4, 32}
    assert {q["SN"] for q in p.values()} == {1, 2, 16}
    assert {q["NG"] for c, q in p.items() if c != PC.HOST_SPLIT} == {1, 2, 3, 8}
    a = p[(70, 1601, 6, 2)]
    assert (a["S"], a["dper"], a["SN"], a["KS"]) == (4, 401, 1, 2) and a["dper"] % 16
    b = p[(513, 513, 17, 9)]
    assert (b["S"], b["dper"], b["SN"], b["tper"], b["nblk"], b["NG"], b["EG"]) == (2, 257, 2, 5, 9, 3, 4)
    assert (b["KS"], b["tail_len"], b["LTM"]) == (5, 1, 1) and b["dper"] % 16 and b["lds_optin"]
    c = p[(8193, 20, 20, 5)]
    assert (c["SN"], c["tper"], c["nblk"], c["empty_spot_slices"], c["NG"]) == (16, 9, 129, [15], 2) and 5 % c["EG"] == 1
    d = p[(64, 16385, 5, 1)]
    assert (d["S"], d["dper"]) == (32, 513) and PC.cdiv(16385, 512) == 33 and PC.cdiv(1536, 1) > 33      # the cap, not smax
    e = p[(200, 149, 36, 9)]
    assert (e["KS"], e["tail_len"], e["NG"], e["nblk"]) == (9, 4, 3, 4)
    assert [p[(200, 70, 20, E)]["NG"] for E in (4, 8, 12, 32)] == [1, 2, 3, 8]
    assert all(not q["empty_gene_slices"] for q in p.values())
    assert [k for k, q in p.items() if q["empty_spot_slices"]] == [(8193, 20, 20, 5)]
    h = p[PC.HOST_SPLIT]
    assert h["split"] == [(32, 32 / 65), (32, 32 / 65), (1, 1 / 65)] and h["ee"] == 32 and h["NG"] == 8
    assert PC.host_split(33) == [(32, 32 / 33), (1, 1 / 33)] and PC.host_split(32) == [(32, 1.0)]


def _library_cases():
    out = set(PC.FACTOR_SWEEP) | set(PC.INSTANCE_ENDS) | set(PC.TILE_EDGES) | set(PC.PLAN_CASES) | {PC.LARGE, PC.SMALL}
    out |= {(130, 80, 20, 32), (130, 80, 20, 1), (130, 80, 20, 3), (3001, 1000, 40, 8), (7000, 17702, 20, 3)}
    return sorted(out)


def test_workspace_bytes_match_the_library():
    """Ties the restated S, SN and slab layout to csrc/poisson.hip: any difference in a slice count changes the size."""
    from gpzoo_amd import _lib
    lib = _lib.load()
    for N, D, Lt, E in _library_cases():
        assert PC.workspace_bytes(N, D, Lt, E) == lib.gpz_poisson_nsf_workspace_bytes(N, D, Lt, E), (N, D, Lt, E)
    for bad in ((10, 4, 65, 1), (10, 4, 0, 1), (10, 4, 3, 33), (10, 4, 3, 0), (0, 4, 3, 1), (10, 0, 3, 1)):
        assert lib.gpz_poisson_nsf_workspace_bytes(*bad) == 0, bad


def test_probe_positions_follow_the_plan():
    g = PC.probe_genes(70, 1601, 6, 2)
    for b in (401, 802, 1203):                      # slice boundaries; the 16- and 64-gene boundaries around 401
        assert b - 1 in g and b in g
    assert {0, 1600, 15, 16, 63, 64, 383, 384, 399, 400, 415, 416, 447, 448, 1599}.issubset(g)
    assert {416, 417}.issubset(g)                   # pass A's first group boundary of slice 1: 401 + 16
    assert PC.probe_spots(70, 1601, 6, 2) == [0, 63, 64, 67, 68, 69]
    s = PC.probe_spots(8193, 20, 20, 5)
    assert s == sorted({0, 8191, 8192} | {x for k in range(1, 15) for x in (576 * k - 1, 576 * k)})
    assert PC.probe_spots(513, 513, 17, 9) == [0, 319, 320, 511, 512]
    assert PC.probe_genes(8193, 20, 20, 5) == [0, 15, 16, 19]
    assert PC.probe_positions(1, 1, 1, 1) == [(0, 0)]
    for shape in PROBE_CASES:
        pos = PC.probe_positions(*shape)
        assert {d for d, _ in pos} == set(PC.probe_genes(*shape)) and {n for _, n in pos} == set(PC.probe_spots(*shape))
        assert len(set(pos)) == len(pos)


@pytest.mark.parametrize("shape", PROBE_CASES, ids=lambda s: "x".join(map(str, s)))
def test_every_probe_is_sharp(shape):
    """The condition that lets the usual tolerances catch one dropped element (module docstring).  (64, 16385, 5, 1) is
    required to be sharp in ll (with the lgamma term) and dW only: 16 385 genes per spot dilute one probe in dV, dmean
    and dscale, and 10^6 rate terms dilute its y log(rate) in the value without the term, whatever count of at most
    20 000 it holds; its slice boundaries are covered sharply by the D = 1601 case."""
    c = PC.make_probe_case(*shape)
    N, D = shape[:2]
    assert [(d, n) for d, n, _ in c["probes"]] == PC.probe_positions(*shape)
    for d, n, cnt in c["probes"]:
        assert isinstance(cnt, int) and 1000 <= cnt <= 20000 and float(c["y"][d, n]) == cnt
    assert float(c["y"].max()) <= 20000 and bool((c["y"] == c["y"].round()).all())
    sh = PC.sharpness(c)
    worst = {k: min(s[k] for s in sh) for k in sh[0]}
    print(shape, len(sh), "probes, counts up to", max(p[2] for p in c["probes"]), {k: round(v, 1) for k, v in worst.items()})
    need = PC.required_sharpness(shape)
    assert need == (("ll_lgamma", "dW") if shape == PC.PARTIAL_SHARPNESS else ("ll", "ll_lgamma", "dmean", "dscale", "dW", "dV"))
    for k in need:
        assert worst[k] >= PC.SHARP_NEED == 10.0, (k, worst[k])


def test_probe_delta_is_the_difference_of_two_evaluations():
    c = PC.make_case(70, 37, 20, 2, probes=[(16, 64, 1234), (36, 69, 1500)])
    for with_lgamma in (False, True):
        ref = PC.reference(c, with_lgamma)
        z = dict(c, y=c["y"].clone(), probes=[(36, 69, 1500)])
        z["y"][16, 64] = 0.0
        zer = PC.reference(z, with_lgamma)
        dl = PC.probe_delta(c, 16, 64, with_lgamma)
        assert dl["ll"] == pytest.approx(ref["ll"] - zer["ll"], rel=1e-10)
        diff = {k: ref[k] - zer[k] for k in PC.OUTPUTS}
        kw = dict(rtol=1e-9, atol=1e-9)
        torch.testing.assert_close(dl["dW"], diff["dW"][16], **kw)
        torch.testing.assert_close(dl["dV"], diff["dV"][64], **kw)
        torch.testing.assert_close(dl["dmean"], diff["dmean"][:, 64], **kw)
        torch.testing.assert_close(dl["dscale"], diff["dscale"][:, 64], **kw)
        diff["dW"][16] = 0.0                        # ... and nothing else moves
        diff["dV"][64] = 0.0
        diff["dmean"][:, 64] = 0.0
        diff["dscale"][:, 64] = 0.0
        assert all(float(v.abs().max()) < 1e-9 for v in diff.values())


def test_reference_is_the_poisson_log_density():
    c = PC.make_counts_case()
    rate = c["V"] * torch.matmul(c["W"], torch.exp(c["mean"] + c["scale"] * c["eps"]))
    want = torch.distributions.Poisson(rate, validate_args=False).log_prob(c["y"]).mean(0).sum()
    assert PC.reference(c, True)["ll"] == pytest.approx(float(want), rel=1e-12)
    lg = float(torch.lgamma(c["y"] + 1.0).sum())
    assert PC.reference(c, False)["ll"] - lg == pytest.approx(PC.reference(c, True)["ll"], rel=1e-12)
    for k in PC.OUTPUTS:
        assert torch.equal(PC.reference(c, False)[k], PC.reference(c, True)[k])


def test_reference_gradients_against_central_differences():
    c = PC.make_case(5, 4, 3, 2, probes=[(1, 2, 1000)])
    ref = PC.reference(c, True)
    h = 1e-6
    for name, out in (("mean", "dmean"), ("scale", "dscale"), ("W", "dW"), ("V", "dV")):
        fd = torch.zeros_like(c[name])
        for i in range(c[name].numel()):
            vals = []
            for s in (h, -h):
                m = dict(c, **{name: c[name].clone()})
                m[name].reshape(-1)[i] += s
                vals.append(float(PC._loglik(m["mean"], m["scale"], m["eps"], m["W"], m["V"], m["y"], True)))
            fd.reshape(-1)[i] = (vals[0] - vals[1]) / (2 * h)
        assert float((ref[out] - fd).abs().max()) <= 1e-6 * float(fd.abs().max()), name


@pytest.mark.parametrize("which", ["counts", (70, 1601, 6, 2), (513, 513, 17, 9), (8193, 20, 20, 5), (130, 80, 20, 65),
                                   (70, 37, 20, 2)], ids=str)
def test_fp64_reference_agrees_with_its_fp32_evaluation(which):
    """Guards the reference against a slip that only shows in one precision: the same formula in fp32 torch agrees to
    1e-5 of each output's largest entry."""
    c = PC.make_counts_case() if which == "counts" else PC.make_probe_case(*which) if which in PROBE_CASES else PC.make_case(*which)
    for with_lgamma in (False, True):
        r64, r32 = PC.reference(c, with_lgamma), PC.reference(c, with_lgamma, dtype=torch.float32)
        print(which, with_lgamma, "ll", abs(r32["ll"] - r64["ll"]) / abs(r64["ll"]),
              {k: float((r32[k] - r64[k]).abs().max() / r64[k].abs().max()) for k in PC.OUTPUTS})
        assert abs(r32["ll"] - r64["ll"]) <= 1e-5 * abs(r64["ll"])
        for k in PC.OUTPUTS:
            assert float((r32[k] - r64[k]).abs().max()) <= 1e-5 * float(r64[k].abs().max()), k


def test_case_inputs():
    c = PC.make_case(130, 80, 20, 3)
    for k in ("mean", "scale", "eps", "W", "V", "y"):
        assert c[k].dtype == torch.float64 and torch.equal(c[k], c[k].float().double()), k
    assert c["mean"].shape == (20, 130) and c["eps"].shape == (3, 20, 130) and c["W"].shape == (80, 20)
    assert c["V"].shape == (130,) and c["y"].shape == (80, 130)
    assert float(c["W"].min()) > 0.01 and float(c["V"].min()) > 0 and float(c["scale"].min()) >= 0.2
    assert float(c["W"].max() / c["W"].min()) > 50          # wider than the older tests' rand + 0.05 (a ratio of 21)
    assert torch.equal(c["y"], PC.make_case(130, 80, 20, 3)["y"]) and not torch.equal(c["y"], PC.make_case(130, 80, 20, 3, seed=1)["y"])
    y = PC.make_counts_case()["y"]
    for v in PC.COUNT_VALUES:
        assert bool((y == v).any()), v
    assert not y[17].any() and not y[:, 66].any() and float(y[1, 129]) == 12345.0
    assert bool((y[:, 128:] > 255).any())                   # the lgammaf branch also in the ragged last tile
