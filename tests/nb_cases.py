"""Cases and fp64 oracle of the negative-binomial step (gpz_nb_nsf), shared by tests/test_hip_nb.py (GPU) and
tests/test_nb_cases.py (CPU: the list covers every kernel instance, both alignment paths and every listed extent).

The oracle is torch's own density: autograd in fp64 on the CPU through
``NegativeBinomial(total_count=theta[:, None], logits=log(rate) - log(theta[:, None])).log_prob(y).mean(0).sum()``."""
import math

import numpy as np
import torch

# extents the sweep must visit (tile edge 64 and N % 4 != 0 among the spots; one 16-gene group, a ragged one, more than
# one 64-gene block and one gene past four blocks among the genes; one sample, a partial and more than one LDS group of 4)
GENES = (1, 7, 130, 257)
SPOTS = (1, 63, 64, 65, 500)
SAMPLES = (1, 3, 5)
FACTORS_REQUIRED = (1, 4, 5, 20, 33, 40, 64)

# (D, N, Lt, E, with_lgamma, why)
SWEEP = [
    (1, 1, 1, 1, True, "the smallest problem; lowest factor count of instance 1..4"),
    (7, 63, 4, 3, False, "highest of 1..4; one ragged tile, rows not 16-byte aligned"),
    (130, 64, 5, 1, True, "lowest of 5..8; exactly one full aligned tile, three 64-gene blocks"),
    (257, 65, 8, 5, False, "highest of 5..8; a tile plus one spot, unaligned rows, two LDS sample groups"),
    (7, 500, 9, 3, True, "lowest of 9..16; eight tiles, the last ragged, aligned rows"),
    (130, 63, 16, 1, False, "highest of 9..16; unaligned rows with a ragged gene group"),
    (257, 500, 17, 3, True, "lowest of 17..20: one factor row on the vector tail of the gene pass"),
    (130, 500, 20, 5, False, "highest of 17..20, the notebooks' factor count; five samples"),
    (1, 64, 21, 3, True, "lowest of 21..24; a single gene"),
    (7, 65, 24, 1, False, "highest of 21..24; unaligned rows"),
    (130, 1, 25, 5, True, "lowest of 25..32; a single spot"),
    (257, 64, 32, 3, False, "highest of 25..32; no padded factor slot at all"),
    (7, 64, 33, 5, True, "lowest of 33..40"),
    (130, 65, 40, 3, False, "highest of 33..40, the notebooks' hybrids (20 + 20)"),
    (257, 63, 41, 1, True, "lowest of 41..48; unaligned rows with three factor tiles"),
    (1, 500, 48, 3, False, "highest of 41..48; a single gene over many tiles"),
    (130, 500, 49, 1, True, "lowest of 49..64"),
    (257, 500, 64, 3, False, "highest of 49..64: the factor limit at the largest extents of the sweep"),
    (7, 1, 64, 5, True, "the factor limit on a single spot, two LDS sample groups"),
    (257, 1, 20, 3, False, "a single spot under every gene block"),
]

# (D, N, Lt, E): the lowest and the highest factor count of each of the nine kernel instances on the smallest shape that has
# both paths of both passes in one launch -- N = 68 is a multiple of 4 (the 16-byte paths), spot tile 0 is full (the
# interior branch) and tile 1 holds 4 spots (the masked branch), gene groups 0..15 and 16..31 are full and 32..39 is
# partial; one gene slice, one spot slice
INSTANCE_ENDS = [(40, 68, Lt, 2) for Lt in (1, 4, 5, 8, 9, 16, 17, 20, 21, 24, 25, 32, 33, 40, 41, 48, 49, 64)]


def make_inputs(D, N, Lt, E, seed, theta=None):
    """Inputs built like test_random_poisson_shapes; theta log-spaced over [0.3, 50] across the genes (or the given value
    for all of them); y gamma-Poisson with mean rate 0.3 .. 2 -- many zeros, some counts >= 16 -- and one entry of 300."""
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    mean = 0.3 * torch.randn(Lt, N, generator=g)
    scale = 0.2 + 0.3 * torch.rand(Lt, N, generator=g)
    eps = torch.randn(E, Lt, N, generator=g)
    W = torch.rand(D, Lt, generator=g) + 0.05
    V = 0.5 + torch.rand(N, generator=g)
    if theta is None:
        th = torch.logspace(math.log10(0.3), math.log10(50.0), D) if D > 1 else torch.tensor([0.3])
    else:
        th = torch.full((D,), float(theta))
    rate = 0.3 + 1.7 * rng.random((D, N))
    shape = th.double().numpy()[:, None]
    y = torch.from_numpy(rng.poisson(rng.gamma(shape, rate / shape)).astype(np.float32))
    y[0, 0] = 300.0
    return dict(mean=mean, scale=scale, eps=eps, W=W, V=V, theta=th.float(), y=y)


def oracle(c, with_lgamma=True):
    """(value, dict of the five gradients + dmean's sibling) in fp64 on the CPU."""
    lv = {k: c[k].double().requires_grad_(True) for k in ("mean", "scale", "W", "V", "theta")}
    yd = c["y"].double()
    rate = lv["V"] * torch.matmul(lv["W"], torch.exp(lv["mean"] + lv["scale"] * c["eps"].double()))
    th = lv["theta"][:, None]
    lp = torch.distributions.NegativeBinomial(total_count=th, logits=torch.log(rate) - torch.log(th),
                                              validate_args=False).log_prob(yd)
    if not with_lgamma:
        lp = lp + torch.lgamma(yd + 1.0)
    ref = lp.mean(0).sum()
    ref.backward()
    return float(ref.detach()), {k: v.grad for k, v in lv.items()}


def run(c, with_lgamma=True):
    """The fused step on the GPU: (loglik, dict of gradients keyed like the oracle's)."""
    from gpzoo_amd import ops
    out = ops.nb_nsf(c["mean"].cuda(), c["scale"].cuda(), c["eps"].cuda(), c["W"].cuda(), c["V"].cuda(), c["theta"].cuda(),
                     c["y"].cuda(), with_lgamma)
    return out[0], dict(zip(("mean", "scale", "W", "V", "theta"), out[1:]))


def check(got_ll, got, ref, grads, tag, theta_atol=None):
    """The dense Poisson step's tolerances (tests/test_hip_poisson.py): value rel 5e-5 / abs 1e-3, each gradient rtol 1e-3
    with atol 1e-3 max |oracle gradient|; ``theta_atol`` (per gene) replaces dtheta's atol."""
    import pytest
    print(tag, "value", float(got_ll), "oracle", ref)
    for k, want in grads.items():
        err = (got[k].double().cpu() - want).abs()
        print(f"  d{k}: max err {float(err.max()):.3e}, max |oracle| {float(want.abs().max()):.3e}")
    assert float(got_ll) == pytest.approx(ref, rel=5e-5, abs=1e-3), tag
    for k, want in grads.items():
        g = got[k].double().cpu()
        if k == "theta" and theta_atol is not None:
            bound = theta_atol + 1e-3 * want.abs()
            assert bool(((g - want).abs() <= bound).all()), f"dtheta {tag}: {((g - want).abs() / bound).max()} of the bound"
            continue
        sc = float(want.abs().max()) + 1e-30
        torch.testing.assert_close(g, want, rtol=1e-3, atol=1e-3 * sc, msg=lambda m: f"d{k} {tag}: {m}")
