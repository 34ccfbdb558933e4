"""CPU: the case lists, the restated launch arithmetic and the fp64 references of tests/entry_cases.py are what
tests/test_hip_kernel_entries.py and tests/test_hip_precomputed.py take them for -- the lists reach every store variant,
column tail, latent split, kgrad tail class, finish side, Mp and chunking they claim; the precomputed recipe holds its clamp
conditions; the references agree with central differences; every probe column and every chunk is *sharp* (dropping it
moves a reference output by at least ten tolerances of the GPU comparison); and the references' own arithmetic in fp32
stays inside the fp32 tolerances, so those tolerances are not consumed by the problem itself."""
import pytest
import torch

import entry_cases as E

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def grad_cases():
    return E.grad_cases()


@pytest.fixture(scope="module")
def pre_cases():
    out = [(f"{s}-{'clamped' if cl else 'free'}", E.precomputed_case(*s, clamped=cl)) for s in E.PRE_SHAPES for cl in (True, False)]
    out += [(f"chunk-{N}-{M}", c) for N, M, w, c in E.chunk_cases() if w == E.CHUNK_WIDTHS[0]]
    out += [("shared", E.precomputed_case(3, 129, 33, shared=True)),
            ("shared-scalar", E.precomputed_case(3, 129, 33, shared=True, scalar_sigma=True))]
    return out


def test_fill_lists_reach_every_variant_tail_and_split():
    plans = E.fill_plans()
    for vec_ok in (True, False):      # both store variants, each with one and with more than one column block, per output type
        for VEC in (4, 2):
            assert any(p["vec_ok"] == vec_ok and p["col_blocks"] == 1 and p["VEC"] == VEC for _, p in plans)
            assert any(p["vec_ok"] == vec_ok and p["col_blocks"] > 1 and p["VEC"] == VEC for _, p in plans)
    assert {p["col_tail"] for _, p in plans if p["VEC"] == 4} == {0, 1, 2, 3}
    assert {p["col_tail"] for _, p in plans if p["VEC"] == 2} == {0, 1}
    assert any(p["row_blocks"] > 1 for _, p in plans)
    for kind in ("rbf", "mggp"):
        sp = [p for k, p in plans if k == kind and "L" in p and p["lmax"] > 1]
        assert any(p["L"] <= p["lmax"] and p["launches"] == 1 for p in sp)
        assert any(p["L"] == p["lmax"] + 1 and p["launches"] == 2 for p in sp)
        assert any(p["L"] > 2 * p["lmax"] and p["launches"] == 3 for p in sp)
    assert E.kfill_plan("mggp", 227, 5, 9, False, G=3)["lmax"] == 227 and E.kfill_plan("mggp", 3, 5, 9, False, G=8)["lmax"] == 32
    g45 = E.kfill_plan("mggp", 3, 5, 9, False, G=45)
    assert g45["lmax"] == 1 and g45["launches"] == 3 and 46 * 46 > E.KF_MAXTAB
    for G in (8, 45):                 # the split cases index the last entry of the (G, G) table
        c = E.kernel_case("mggp", 2, *E.SPLIT_SHAPE, L=3, G=G)
        assert int((c["gA"][:, None] * G + c["gB"][None, :]).max()) == G * G - 1 and int(c["gA"].min()) == 0
    # the C ABI grid: every reason for the scalar-store variant on its own, and the aligned window of a padded matrix
    assert not E.kfill_plan("rbf", 2, 3, 8, False, ldk=8, stride=24, base_off=1)["vec_ok"]
    assert not E.kfill_plan("rbf", 2, 3, 8, False, ldk=9, stride=27)["vec_ok"]
    assert not E.kfill_plan("rbf", 2, 3, 8, False, ldk=8, stride=29)["vec_ok"]
    assert E.kfill_plan("rbf", 2, 3, 8, False, ldk=12, stride=36)["vec_ok"]
    assert E.kfill_plan("rbf", 2, 3, 8, True, ldk=12, stride=36)["vec_ok"]
    assert E.kfill_plan("rbf", 1, *E.TALL, False)["row_blocks"] == 65537


def test_grad_lists_reach_every_tail_class_and_both_finish_sides(grad_cases):
    classes = {E.kgrad_tail_class(nB) for nB in E.GRAD_SWEEP_NB}
    assert classes == {(False, 1, "one"), (False, 1, "ragged"), (False, 1, "full"), (False, 2, "one"), (False, 3, "ragged"),
                       (False, 4, "ragged"), (False, 4, "full"), (True, 1, "one"), (True, 4, "ragged"), (True, 4, "full")}
    assert {E.kgrad_plan(nB)["trips"] for nB in E.GRAD_SWEEP_NB} == {1, 2, 3, 5}
    assert E.kgrad_plan(E.MAIN_GRAD[1]) == dict(trips=2, slots=1, tail=1)
    assert [E.kgrad_finish_fx(nA, L) for nA, _, L in E.FINISH_CASES] == [(5, "rows"), (7, "latents")]
    assert {c["kind"] for _, c in grad_cases} == set(E.GRAD_KINDS)
    assert {(c["kind"], c["d"]) for n, c in grad_cases if n.startswith("main")} == {(k, d) for k in E.GRAD_KINDS for d in (1, 2, 3, 4)}
    for _, c in grad_cases:           # distinct per-latent parameters
        for n in ("sigma", "ell") + (("a",) if c["a"] is not None else ()):
            assert c[n].unique().numel() == c["L"]
    c = E.kernel_case("mggp", 2, 9, 261)
    assert c["gA"].unique().numel() == 5 and c["gB"].unique().numel() == 5
    assert E.per_latent(E.SIG, 600).unique().numel() == 600 and float(c["A"].abs().max()) <= 4


def test_probe_columns():
    assert E.probe_columns(1) == [0] and E.probe_columns(64) == [0, 63] and E.probe_columns(65) == [0, 63, 64]
    assert E.probe_columns(257) == [0, 63, 64, 127, 128, 191, 192, 255, 256]
    c = E.kernel_case("rbf", 2, 3, 257)
    up = E.upstreams(c)["probe"]
    on = (up != 0).any(0).any(0).nonzero().reshape(-1).tolist()
    assert on == E.probe_columns(257) and 0.75 <= float(up[:, :, on].abs().min()) and float(up.abs().max()) <= 1.25


def test_precomputed_lists_reach_every_pad_and_chunking():
    assert {E.pre_plan(L, N, M, 4)["Mp"] for L, N, M in E.PRE_SHAPES} == {128, 256, 384}
    assert all(E.pre_plan(L, N, M, e)["nchunks"] == 1 for L, N, M in E.PRE_SHAPES for e in (4, 8))    # the rule never cuts here
    # BASELINE config 3 sizes (N = 200 000, M = 2048, L = 32, fp32): there the rule cuts, so the chunk loop is the usual path
    big = E.pre_plan(32, 200000, 2048, 4)
    assert big["nc"] == 8192 and big["nchunks"] == 25 and E.pre_plan(256, 200000, 2048, 4)["nc"] == 1024
    seen = set()
    for N, M, w, c in E.chunk_cases():
        p = E.pre_plan(2, N, M, 4, w)
        cols = E.chunk_columns(N, w)
        assert len(cols) == p["nchunks"] and cols[-1][1] - cols[-1][0] == p["last"] and cols[0][0] == 0 and cols[-1][1] == N
        seen.add((p["nchunks"], "exact" if p["last"] == p["nc"] else "one" if p["last"] == 1 else "ragged"))
    assert {(1, "exact"), (2, "exact"), (3, "ragged"), (3, "one"), (2, "one")} <= seen
    assert {E.pre_plan(2, 300, M, 4, 128)["Mp"] for M in E.CHUNK_M} == {128, 384}
    assert E.pre_plan(2, 300, 33, 4, 128)["ncp_last"] == 128 and E.pre_plan(2, 300, 33, 4, 256)["nc"] == 256


def test_precomputed_recipe_holds_its_conditions(pre_cases):
    for name, c in pre_cases:
        ref = E.precomputed_ref(c)
        prior = ref["prior"]                                # (sigma^2 - sum W^2) / sigma^2
        assert float(prior.abs().min()) >= 0.3, name       # clamp margin
        share = (prior < 0).double().mean(-1)
        if not c["clamped"]:
            assert float(share.max()) == 0.0, name
        elif c["N"] >= 4:
            assert 0.4 <= float(share.min()) and float(share.max()) <= 0.6, name
        assert float(ref["scale"].min()) > 0.1, name
        want = {0.75, 0.36, -0.5625, -1.56} if c["clamped"] else {0.75, 0.36}
        assert all(min(abs(v - w) for w in want) < 1e-5 for v in prior.reshape(-1).tolist()), name


def _central(f, x, h=1e-6):
    g = torch.zeros_like(x)
    flat, gf = x.reshape(-1), g.reshape(-1)
    for i in range(flat.numel()):
        old = float(flat[i])
        flat[i] = old + h
        up = float(f())
        flat[i] = old - h
        dn = float(f())
        flat[i] = old
        gf[i] = (up - dn) / (2 * h)
    return g


# central differences at h = 1e-6 on O(1) smooth functions: truncation h^2 f''' ~ 1e-12, rounding eps / h ~ 1e-10
CD_TOL = 1e-7


@pytest.mark.parametrize("kind", E.GRAD_KINDS)
@pytest.mark.parametrize("shape", [(3, 4, 2), (2, 5, 3)])
def test_kernel_gradient_reference_against_central_differences(kind, shape):
    nA, nB, d = shape
    c = E.kernel_case(kind, d, nA, nB)
    Kbar = E.upstreams(c)["dense"]
    ref = E.kernel_grads(c, Kbar)
    x = {n: c[n].clone() for n in ("A", "sigma", "ell") + (("a",) if c["a"] is not None else ())}
    f = lambda: (E.kernel_value(c, x["A"], c["B"], x["sigma"], x["ell"], x.get("a")) * Kbar).sum()
    got = {n: _central(f, t) for n, t in x.items()}
    theta = torch.stack([got["sigma"], got["ell"], got.get("a", torch.zeros(c["L"], dtype=F64))], 1)
    for a, b in ((theta, ref["theta"]), (got["A"], ref["A"])):
        assert float((a - b).abs().max()) <= CD_TOL * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("clamped", [True, False])
@pytest.mark.parametrize("shape", [(2, 5, 3), (1, 4, 2)])
def test_precomputed_reference_against_central_differences(shape, clamped):
    c = E.precomputed_case(*shape, clamped=clamped)
    ref = E.precomputed_ref(c)
    for n, gn in (("mu", "grad_mu"), ("Lu_raw", "grad_Lu"), ("sigma", "grad_sigma")):
        got = _central(lambda: E.precomputed_ref(c)["loss"], c[n])
        assert float((got - ref[gn]).abs().max()) <= CD_TOL * max(1.0, float(ref[gn].abs().max())), n


def test_every_probe_column_is_sharp(grad_cases):
    """Zeroing the probe upstream in any single boundary column moves at least one reference output by at least ten times
    that output's (fp32, the wider) tolerance.  The gradients are linear in the upstream: the move is the column's own term."""
    worst = (float("inf"), None)
    for name, c in grad_cases:
        up = E.upstreams(c)["probe"]
        ref = E.kernel_grads(c, up)
        tol = {n: E.grad_tol(ref[n], F32) for n in ("theta", "A")}
        for col in E.probe_columns(c["nB"]):
            only = torch.zeros_like(up)
            only[:, :, col] = up[:, :, col]
            term = E.kernel_grads(c, only)
            ratio = max(float((term[n].abs() / tol[n]).max()) for n in ("theta", "A"))
            worst = min(worst, (ratio, f"{name} column {col}"))
    assert worst[0] >= 10.0, worst


def test_every_chunk_is_sharp():
    """Dropping any single chunk's columns from the reference moves the Lu gradient by at least ten (fp32) tolerances.  A last
    chunk of ONE column does not do that under the plain recipe (its term is 1/N of the diagonal's sum); the cases whose last
    chunk is one column multiply the upstreams of that column by BOOST_ONE_COLUMN."""
    for N, M, w, c in E.chunk_cases():
        cols = E.chunk_columns(N, w)
        if len(cols) == 1:
            continue
        full = E.precomputed_ref(c)["grad_Lu"]
        tol = E.pre_tol(full, F32)
        for a, b in cols:
            keep = torch.tensor([n for n in range(N) if not a <= n < b], dtype=torch.long)
            part = E.precomputed_ref(c, keep=keep)["grad_Lu"]
            assert float(((full - part).abs() / tol).max()) >= 10.0, (N, M, w, a, b)
    plain = E.precomputed_case(2, 257, 33)
    full = E.precomputed_ref(plain)["grad_Lu"]
    part = E.precomputed_ref(plain, keep=torch.arange(256))["grad_Lu"]
    assert float(((full - part).abs() / E.pre_tol(full, F32)).max()) < 10.0       # why the boost is there


def test_kernel_references_in_fp32_stay_inside_the_fp32_tolerances(grad_cases):
    for name, c in grad_cases:
        for un, up in E.upstreams(c).items():
            ref, low = E.kernel_grads(c, up), E.kernel_grads(c, up, dtype=F32)
            for n in ("theta", "A"):
                r = float(((low[n].double() - ref[n]).abs() / E.grad_tol(ref[n], F32)).max())
                assert r <= 1.0, (name, un, n, r)
    for kind in E.KINDS:
        for d in (1, 2, 3, 4):
            c = E.kernel_case(kind, d, *E.MAIN_FILL)
            K = E.kernel_value(c)
            K32 = E.kernel_value(c, *(c[n].float() for n in ("A", "B", "sigma", "ell")), None if c["a"] is None else c["a"].float())
            torch.testing.assert_close(K32.double(), K, rtol=1e-4, atol=1e-4)


def test_precomputed_reference_in_fp32_stays_inside_the_fp32_tolerances(pre_cases):
    for name, c in pre_cases:
        ref, low = E.precomputed_ref(c), E.precomputed_ref(c, dtype=F32)
        for n in ("mean", "scale", "grad_mu", "grad_Lu", "grad_sigma"):
            r = float(((low[n].double() - ref[n]).abs() / E.pre_tol(ref[n], F32, relative_only=n == "scale")).max())
            assert r <= 1.0, (name, n, r)
