"""GPU: the fused negative-binomial step (gpz_nb_nsf, ops.nb_nsf) against fp64 CPU autograd through
torch.distributions.NegativeBinomial -- every kernel instance, tile edge and alignment path (tests/nb_cases.py), the
host's split at 32 samples, the Poisson limit, counts that all take the lgamma / digamma branch, bitwise
reproducibility and the refusals.  Tolerances are the dense Poisson step's (tests/test_hip_poisson.py)."""
import pytest
import torch

import nb_cases as NC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("i", range(len(NC.SWEEP)))
def test_nb_sweep(i):
    D, N, Lt, E, with_lgamma, why = NC.SWEEP[i]
    c = NC.make_inputs(D, N, Lt, E, seed=1300 + i)
    ref, grads = NC.oracle(c, with_lgamma)
    ll, got = NC.run(c, with_lgamma)
    NC.check(ll, got, ref, grads, dict(D=D, N=N, Lt=Lt, E=E, with_lgamma=with_lgamma, why=why))


@pytest.mark.parametrize("D,N,Lt,E", NC.INSTANCE_ENDS, ids=["Lt%d" % c[2] for c in NC.INSTANCE_ENDS])
def test_nb_instance_ends(D, N, Lt, E):
    """Both ends of every kernel instance, each with the interior and the masked branch of both passes in one launch."""
    c = NC.make_inputs(D, N, Lt, E, seed=1500 + Lt)
    ref, grads = NC.oracle(c, True)
    ll, got = NC.run(c, True)
    NC.check(ll, got, ref, grads, dict(D=D, N=N, Lt=Lt, E=E))


def test_host_split_counts_the_sample_independent_terms_once():
    """E = 33 goes through two calls (32 + 1); lgamma(y + theta) - lgamma(theta), the psi terms of dtheta and lgamma(y + 1)
    do not depend on the sample and must enter the value and dtheta once."""
    c = NC.make_inputs(70, 300, 20, 33, seed=1401)
    ref, grads = NC.oracle(c, True)
    ll, got = NC.run(c, True)
    NC.check(ll, got, ref, grads, "E=33")


def test_near_poisson_limit():
    """theta = 1e4 for every gene: dtheta's terms cancel to O(1 / theta^2), so its absolute tolerance is 1e-3 of what
    cancels, sum_n |psi(y + theta) - psi(theta)| per gene from the oracle; the value lies within D N max(mu)^2 / theta of the
    Poisson oracle's."""
    D, N, Lt, E = 37, 65, 5, 3
    c = NC.make_inputs(D, N, Lt, E, seed=1402, theta=1e4)
    ref, grads = NC.oracle(c, True)
    ll, got = NC.run(c, True)
    yd, th = c["y"].double(), c["theta"].double()[:, None]
    cancels = (torch.digamma(yd + th) - torch.digamma(th)).abs().sum(1)
    NC.check(ll, got, ref, grads, "theta=1e4", theta_atol=1e-3 * cancels)
    rate = c["V"].double() * torch.matmul(c["W"].double(), torch.exp(c["mean"].double() + c["scale"].double() * c["eps"].double()))
    poi = float(torch.distributions.Poisson(rate, validate_args=False).log_prob(yd).mean(0).sum())
    bound = D * N * float(rate.max()) ** 2 / 1e4
    print("NB", float(ll), "Poisson oracle", poi, "bound", bound)
    assert abs(float(ll) - poi) <= bound, (float(ll), poi, bound)


def test_large_counts_only():
    """y >= 16 everywhere and one row of non-integer counts: every element takes lgamma and the digamma series."""
    D, N, Lt, E = 9, 70, 5, 2
    c = NC.make_inputs(D, N, Lt, E, seed=1403)
    g = torch.Generator().manual_seed(1403)
    c["y"] = 16.0 + torch.poisson(20.0 * torch.rand(D, N, generator=g), generator=g)
    c["y"][3] += 0.5
    assert float(c["y"].min()) >= 16.0
    for with_lgamma in (True, False):
        ref, grads = NC.oracle(c, with_lgamma)
        ll, got = NC.run(c, with_lgamma)
        NC.check(ll, got, ref, grads, f"y>=16 with_lgamma={with_lgamma}")


def test_two_calls_agree_bit_for_bit():
    c = NC.make_inputs(130, 500, 20, 3, seed=1404)
    ll1, g1 = NC.run(c, True)
    ll2, g2 = NC.run(c, True)
    assert torch.equal(ll1, ll2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_factor_count_limit_is_reported():
    from gpzoo_amd import ops
    Lt, N, D = 65, 10, 4
    with pytest.raises((RuntimeError, ValueError), match="65 factors unsupported"):
        ops.nb_nsf(torch.zeros(Lt, N).cuda(), torch.ones(Lt, N).cuda(), torch.zeros(1, Lt, N).cuda(),
                   torch.ones(D, Lt).cuda(), torch.ones(N).cuda(), torch.ones(D).cuda(), torch.ones(D, N).cuda())


def test_sparse_counts_are_refused():
    from gpzoo_amd import ops
    from gpzoo_amd.likelihoods import SparseCounts
    Lt, N, D = 3, 10, 4
    y = SparseCounts(torch.eye(D, N)).cuda()
    with pytest.raises(TypeError, match="dense counts.*to_dense"):
        ops.nb_nsf(torch.zeros(Lt, N).cuda(), torch.ones(Lt, N).cuda(), torch.zeros(1, Lt, N).cuda(),
                   torch.ones(D, Lt).cuda(), torch.ones(N).cuda(), torch.ones(D).cuda(), y)
