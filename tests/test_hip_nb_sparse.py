"""GPU: the sparse negative-binomial step (gpz_nb_nsf_sparse, ops.nb_nsf_sparse, csrc/nb_sparse.hip) against fp64 CPU
autograd through torch.distributions.NegativeBinomial on the batch's dense counts (tests/sparse_nb_cases.py;
tests/test_sparse_nb_cases.py checks the cases, the probes and the decomposition on the CPU).

Bounds: nb_cases.check's -- value rel 5e-5 / abs 1e-3, gradients rtol 1e-3 with atol 1e-3 max |oracle| -- with dtheta's
absolute bound at theta = 1e4 being 1e-3 sum_n |psi(y + theta) - psi(theta)| per gene, as test_hip_nb.py's
test_near_poisson_limit has it.  Every case runs with and without the lgamma(y + 1) term; nb_cases.check prints each
figure before it asserts."""
import pytest
import torch

import nb_cases as NC
import sparse_nb_cases as SN

pytestmark = pytest.mark.gpu

CASES = SN.all_cases()
BY_NAME = dict(CASES)


def _params(c):
    return [c[k].float().cuda() for k in ("mean", "scale", "eps", "W", "V", "theta")]


def counts_of(c):
    """The case's SparseCounts on the GPU (the batch view for a batch case).  Positions listed in c["stored_zeros"] are
    stored entries whose value is 0."""
    from gpzoo_amd.likelihoods import SparseCounts
    y = c["y"].float().clone()
    for d, n in c["stored_zeros"]:
        y[d, n] = 1.0
    s = SparseCounts(y)
    for d, n in c["stored_zeros"]:
        k0, k1 = int(s.col_ptr[n]), int(s.col_ptr[n + 1])
        k = k0 + s.col_gene[k0:k1].tolist().index(d)
        s.col_val[k] = 0.0
    assert int((s.col_val == 0).sum()) == len(c["stored_zeros"])
    s = s.cuda()
    return s[:, c["idx"].cuda()] if "idx" in c else s


def run(c, with_lgamma, counts=None, **kw):
    from gpzoo_amd import ops
    out = ops.nb_nsf_sparse(*_params(c), counts_of(c) if counts is None else counts, with_lgamma=with_lgamma, **kw)
    assert out[0].dtype == torch.float64 and all(t.dtype == torch.float32 for t in out[1:])
    assert all(bool(torch.isfinite(t).all()) for t in out)
    return out


def check(c, out, with_lgamma, tag, theta_atol=None):
    ref, grads = SN.reference(c, with_lgamma)
    NC.check(out[0], dict(zip(SN.GRADS, out[1:])), ref, grads, f"{tag} with_lgamma={with_lgamma}", theta_atol=theta_atol)


@pytest.mark.parametrize("name", [n for n, _ in CASES if n != "poisson_limit"])
def test_case_against_oracle(name):
    """Every case of the list, with and without the lgamma term; the gradients do not depend on it, bit for bit."""
    c = BY_NAME[name]
    counts = counts_of(c)
    plain, full = run(c, False, counts), run(c, True, counts)
    check(c, plain, False, name)
    check(c, full, True, name)
    for k, a, b in zip(SN.GRADS, plain[1:], full[1:]):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("shape", SN.INSTANCE_END_SHAPES, ids=["Lt%d" % s[2] for s in SN.INSTANCE_END_SHAPES])
def test_zero_part_instance_ends(shape):
    """Both ends of every kernel instance of the zero part, each with the interior and the masked branch of both passes."""
    c = SN.instance_end_case(shape)
    check(c, run(c, True), True, "ends-" + SN._shape_id(shape))


def test_near_poisson_limit():
    c = BY_NAME["poisson_limit"]
    atol = SN.poisson_limit_theta_atol(c)
    for with_lgamma in (False, True):
        check(c, run(c, with_lgamma), with_lgamma, "theta=1e4", theta_atol=atol)


def test_no_counts_equals_the_dense_step_on_zeros():
    from gpzoo_amd import ops
    c = SN.no_counts_case()
    sparse = run(c, True)
    dense = ops.nb_nsf(*_params(c), torch.zeros(c["y"].shape, device="cuda"), True)
    _, grads = SN.reference(c, True)
    assert float(sparse[0]) == pytest.approx(float(dense[0]), rel=SN.LL_REL, abs=SN.LL_ABS)
    for k, a, b in zip(SN.GRADS, sparse[1:], dense[1:]):
        torch.testing.assert_close(a, b, rtol=SN.G_RTOL, atol=SN.G_ATOL * float(grads[k].abs().max()), msg=lambda m: f"d{k}: {m}")


@pytest.mark.parametrize("name", ["batch_B70", "batch_perm", "batch_empty_cols"])
def test_idx_and_view_give_equal_bits(name):
    from gpzoo_amd.likelihoods import SparseCounts
    c = BY_NAME[name]
    base = SparseCounts(c["y"].float()).cuda()
    idx = c["idx"].cuda()
    by_view, by_idx = run(c, True, base[:, idx]), run(c, True, base, idx=idx)
    for a, b in zip(by_view, by_idx):
        assert torch.equal(a, b)


def test_two_calls_agree_bit_for_bit():
    c, other = SN.chunk_case(), SN.batch_case("B70")
    counts, counts_other = counts_of(c), counts_of(other)
    first = run(c, True, counts)
    second = run(c, True, counts)
    run(other, True, counts_other)                     # another problem writes the same workspace
    third = run(c, True, counts)
    for a, b, d in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, d)


def test_side_stream_does_not_disturb_the_default_stream():
    c, other = SN.shape_case(SN.FACTOR_SHAPES[3]), SN.batch_case("B70")
    counts, counts_other = counts_of(c), counts_of(other)
    want = run(c, True, counts)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got = run(c, True, counts)
    with torch.cuda.stream(side):
        on_side = run(other, True, counts_other)
    torch.cuda.synchronize()
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    check(other, on_side, True, "side stream")


def test_refusals():
    from gpzoo_amd import ops
    from gpzoo_amd.likelihoods import SparseCounts
    c = SN.one_count_case()
    mean, scale, eps, W, V, th = _params(c)
    counts = counts_of(c)
    D, N = c["y"].shape
    with pytest.raises((RuntimeError, ValueError), match=r"gpz_nb_nsf_sparse\w*: 65 factors unsupported"):
        ops.nb_nsf_sparse(torch.zeros(65, N).cuda(), torch.ones(65, N).cuda(), torch.zeros(1, 65, N).cuda(),
                          torch.ones(D, 65).cuda(), V, th, counts)
    with pytest.raises(TypeError, match="SparseCounts"):
        ops.nb_nsf_sparse(mean, scale, eps, W, V, th, c["y"].float().cuda())
    with pytest.raises(RuntimeError, match="counts live on"):
        ops.nb_nsf_sparse(mean, scale, eps, W, V, th, SparseCounts(c["y"].float()))
    for bad in (dict(V=V[:-1]), dict(th=th[:-1]), dict(W=W[:-1]), dict(eps=eps[:, :-1]), dict(scale=scale[:, :-1])):
        a = dict(mean=mean, scale=scale, eps=eps, W=W, V=V, th=th)
        a.update(bad)
        with pytest.raises(ValueError, match="do not fit together"):
            ops.nb_nsf_sparse(a["mean"], a["scale"], a["eps"], a["W"], a["V"], a["th"], counts)
