"""Cases and fp64 oracle of the Gaussian factor step (gpz_gaussian_fa), shared by tests/test_hip_gaussian.py (GPU) and
tests/test_gaussian_cases.py (CPU: the list covers every kernel instance, both alignment paths, one and several slices of
both passes and every listed extent).

The oracle is autograd in fp64 on the CPU through
``Normal(b[:, None] + W @ mean, sd[:, None]).log_prob(y).sum() - 0.5 * ((W**2 / sd**2[:, None]) @ scale**2).sum()``."""
import functools
import math
from typing import NamedTuple

import torch

import nb_cases as NC

# extents the sweep must visit: nb_cases' genes and spots, and the lowest and highest factor count of each of the
# thirteen kernel instances (1 .. 40 factors in steps of 4, then 41 .. 48, 49 .. 56 and 57 .. 64)
GENES = NC.GENES
SPOTS = NC.SPOTS
FACTORS_REQUIRED = (1, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 32, 33, 36, 37, 40, 41, 48, 49, 56, 57, 64)

# (D, N, Lt, why)
SWEEP = [
    (1, 1, 1, "the smallest problem; lowest factor count of instance 1..4"),
    (7, 63, 4, "highest of 1..4; one ragged tile, rows not 16-byte aligned"),
    (130, 64, 5, "lowest of 5..8; exactly one full aligned tile, three 64-gene blocks"),
    (257, 65, 8, "highest of 5..8; a tile plus one spot, unaligned rows"),
    (7, 500, 9, "lowest of 9..12; eight tiles, the last ragged, aligned rows"),
    (130, 63, 12, "highest of 9..12; unaligned rows with a ragged gene group"),
    (257, 500, 13, "lowest of 13..16"),
    (1, 65, 16, "highest of 13..16; a single gene, unaligned rows"),
    (257, 500, 17, "lowest of 17..20: one factor row in the second 16-row factor tile"),
    (130, 500, 20, "highest of 17..20, the notebooks' factor count"),
    (1, 64, 21, "lowest of 21..24; a single gene"),
    (7, 65, 24, "highest of 21..24; unaligned rows"),
    (130, 1, 25, "lowest of 25..28; a single spot"),
    (257, 63, 28, "highest of 25..28; unaligned rows"),
    (7, 64, 29, "lowest of 29..32"),
    (257, 64, 32, "highest of 29..32; no padded factor slot at all"),
    (7, 64, 33, "lowest of 33..36: the first instance built for one wave per SIMD in the spot pass"),
    (130, 500, 36, "highest of 33..36"),
    (1, 500, 37, "lowest of 37..40; a single gene over many tiles"),
    (130, 65, 40, "highest of 37..40, the notebooks' hybrids (20 + 20)"),
    (257, 63, 41, "lowest of 41..48; unaligned rows with three factor tiles"),
    (7, 500, 48, "highest of 41..48"),
    (130, 500, 49, "lowest of 49..56"),
    (257, 65, 56, "highest of 49..56; unaligned rows"),
    (130, 64, 57, "lowest of 57..64"),
    (257, 500, 64, "highest of 57..64: the factor limit at the largest extents of nb_cases"),
    (7, 1, 64, "the factor limit on a single spot"),
    (257, 1, 20, "a single spot under every gene block"),
    (600, 600, 20, "two gene slices in the spot pass and two spot slices in the gene pass, aligned rows"),
    (530, 601, 7, "two slices of both passes with unaligned rows and ragged edges everywhere"),
]


def make_inputs(D, N, Lt, seed):
    """mean = 0.8 randn, scale in [0.2, 0.5], W ~ randn, b ~ 2 randn, sd log-spaced over [0.05, 3] across the genes,
    y = b + W F + 1.5 sd randn with F drawn from q(F), and one entry of y set to 300."""
    g = torch.Generator().manual_seed(seed)
    mean = 0.8 * torch.randn(Lt, N, generator=g)
    scale = 0.2 + 0.3 * torch.rand(Lt, N, generator=g)
    W = torch.randn(D, Lt, generator=g)
    b = 2.0 * torch.randn(D, generator=g)
    sd = torch.logspace(math.log10(0.05), math.log10(3.0), D) if D > 1 else torch.tensor([0.05])
    F = mean + scale * torch.randn(Lt, N, generator=g)
    y = b[:, None] + W @ F + 1.5 * sd[:, None] * torch.randn(D, N, generator=g)
    y[0, 0] = 300.0
    return dict(mean=mean, scale=scale, W=W, b=b, sd=sd.float(), y=y.float())


@functools.lru_cache(maxsize=None)
def case(i):
    """Inputs of SWEEP[i] and their oracle, built once and shared (treat both as read-only)."""
    D, N, Lt, _ = SWEEP[i]
    c = make_inputs(D, N, Lt, seed=2300 + i)
    return c, oracle(c)


def closed_form(mean, scale, W, b, sd, y):
    """(value, R per gene) of the expected log-likelihood, differentiable, in the dtype of its arguments."""
    r = y - b[:, None] - W @ mean
    val = torch.distributions.Normal(b[:, None] + W @ mean, sd[:, None], validate_args=False).log_prob(y).sum() \
        - 0.5 * ((W ** 2 / (sd ** 2)[:, None]) @ scale ** 2).sum()
    return val, (r ** 2).sum(1)


class Oracle(NamedTuple):
    value: float
    sse: torch.Tensor          # (D,) fp64
    sse_atol: torch.Tensor     # (D,) fp64: what fp32 residuals can cost, see ``oracle``
    grads: dict
    local: dict                # per gradient: the magnitude of its own gene row / spot column, see ``oracle``


def oracle(c):
    """Value, sse per gene and the five gradients in fp64 on the CPU, and the absolute error in sse that any fp32
    evaluation of the residual is allowed.  A residual r = (y - b) - sum_l W m formed in fp32 rounds Lt + 2 times, each
    time by at most 2^-24 of a partial result no larger than T = |y| + |b| + sum_l |W m|, so |dr| <= (Lt + 2) 2^-24 T and
    sse moves by at most sum_n 2 |r| |dr| (to first order).  A relative bound alone cannot hold where a gene's few
    residuals are small next to the terms they are the difference of (N = 1)."""
    lv = {k: c[k].double().requires_grad_(True) for k in ("mean", "scale", "W", "b", "sd")}
    yd = c["y"].double()
    val, sse = closed_form(lv["mean"], lv["scale"], lv["W"], lv["b"], lv["sd"], yd)
    val.backward()
    with torch.no_grad():
        W, m, b = lv["W"].detach(), lv["mean"].detach(), lv["b"].detach()
        r = yd - b[:, None] - W @ m
        T = yd.abs() + b.abs()[:, None] + W.abs() @ m.abs()
        atol = (2.0 * r.abs() * (W.shape[1] + 2) * 2.0 ** -24 * T).sum(1)
        # what each gradient entry is a sum of: the magnitude its own row (gene) or column (spot) reaches, so that the
        # entry of 300 in gene 0, spot 0 -- which sets max |gradient| -- does not hide an error in any other gene or spot
        sd, s = lv["sd"].detach(), lv["scale"].detach()
        grads = {k: v.grad for k, v in lv.items()}
        local = dict(mean=grads["mean"].abs().amax(0, keepdim=True), scale=grads["scale"].abs().amax(0, keepdim=True),
                     W=grads["W"].abs().amax(1, keepdim=True), b=r.abs().sum(1) / sd ** 2,
                     sd=yd.shape[1] / sd + (sse.detach() + (W ** 2 @ (s ** 2).sum(1))) / sd ** 3)
    return Oracle(float(val.detach()), sse.detach(), atol, grads, local)


def torch_fp32(c):
    """The same through torch in fp32 on the CPU: what the number format itself allows."""
    lv = {k: c[k].float().clone().requires_grad_(True) for k in ("mean", "scale", "W", "b", "sd")}
    val, sse = closed_form(lv["mean"], lv["scale"], lv["W"], lv["b"], lv["sd"], c["y"].float())
    val.backward()
    return val.detach(), sse.detach(), {k: v.grad for k, v in lv.items()}


def run(c, grads=True, shift=0):
    """The fused step on the GPU: (loglik, sse, dict of gradients keyed like the oracle's).  ``shift`` > 0 passes every
    input as the view ``t[shift:]`` of a longer buffer (misaligned for shift % 4 != 0)."""
    from gpzoo_amd import ops

    def dev(t):
        if not shift:
            return t.cuda()
        buf = torch.zeros(t.numel() + shift, dtype=t.dtype, device="cuda")
        buf[shift:] = t.reshape(-1).cuda()
        return buf[shift:].view(t.shape)
    out = ops.gaussian_fa(dev(c["mean"]), dev(c["scale"]), dev(c["W"]), dev(c["b"]), dev(c["sd"]), dev(c["y"]), grads=grads)
    return out[0], out[1], dict(zip(("mean", "scale", "W", "b", "sd"), out[2:]))


def check(got_ll, got_sse, got, want: Oracle, tag):
    """nb_cases.check's tolerances (value rel 5e-5 / abs 1e-3, each gradient rtol 1e-3 with atol 1e-3 max |oracle
    gradient|) and sse_per_gene to plain rtol 1e-5.  Only with a single spot (N = 1), where a gene's sse is one squared
    residual and nothing averages its rounding, the oracle's fp32-residual allowance is added per gene."""
    s = got_sse.double().cpu()
    err = (s - want.sse).abs()
    single_spot = want.grads["mean"].shape[1] == 1
    bound = 1e-5 * want.sse.abs() + (want.sse_atol if single_spot else 0.0)
    print(tag, "sse_per_gene: max relative error", float((err / want.sse.abs().clamp_min(1e-300)).max()),
          "largest share of its bound", float((err / bound.clamp_min(1e-300)).max()))
    NC.check(got_ll, got, want.value, want.grads, tag)
    assert bool((err <= bound).all()), f"sse_per_gene {tag}: {float((err / bound.clamp_min(1e-300)).max())} of the bound"
    # beyond nb_cases.check: the same 1e-3, but of the gene's or spot's own magnitude instead of the global maximum
    for k, ref in want.grads.items():
        e = (got[k].double().cpu() - ref).abs()
        lim = 1e-3 * ref.abs() + 1e-3 * want.local[k]
        share = float((e / lim.clamp_min(1e-300)).max())
        print(f"  d{k}: largest share of its own row's / column's bound {share:.3e}")
        assert share <= 1.0, f"d{k} {tag}: {share} of the bound of its own gene / spot"
