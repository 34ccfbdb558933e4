"""Case builders, the restated launch arithmetic and the fp64 reference for tests/test_hip_poisson_forms.py (TEST
INFRASTRUCTURE ONLY; plain torch, importable without a GPU -- tests/test_poisson_cases.py checks everything here on the
CPU).

The operation is the fused Poisson step gpz_poisson_nsf (csrc/poisson.hip):

    ll = (y log(V W exp(mean + scale eps)) - rate [- lgamma(y + 1)]).mean(0).sum()        rate (E,D,N)

and its gradients with respect to mean, scale (Lt,N), W (D,Lt) and V (N,).  A *case* is one (N, D, Lt, E) with seeded
inputs; a *probe* is one large integer count written into y at an element that a wrong bound of the kernels' gene
slices, spot slices, 16-gene groups, 64-spot tiles or 4-spot vector groups would drop or count twice.  ll and every
gradient are sums over (gene, spot) of independent terms, so what one entry of y contributes is known exactly
(``probe_delta``); tests/test_poisson_cases.py asserts that each probe's contribution is at least ten times the
tolerance of the GPU comparison, which is what lets the project's usual tolerances catch a single dropped element.

Every floating-point input is rounded to an fp32-representable value: the kernel and the reference see one problem."""
from __future__ import annotations

import torch

PMAXL, PMAXE, PEG, GS = 64, 32, 4, 4          # csrc/poisson.hip: factors, samples per call, samples per LDS group, waves
NLG = 4096                                    # workgroups (= partial sums) of lgamma_sum_kernel
LL_REL, LL_ABS, G_RTOL, G_ATOL = 5e-5, 1e-3, 1e-3, 1e-3     # tests/test_hip_poisson.py::test_random_poisson_shapes
OUTPUTS = ("dmean", "dscale", "dW", "dV")


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------------------------------------
# the library's own launch arithmetic, restated (csrc/nb_passes.h: slice_plan, pass_b_lds and the LDS opt-in;
# csrc/poisson.hip: poisson_plan, the dispatch switch, poisson_passes, gene_mfma_kernel's constants; csrc/common.h: Carver;
# gpzoo_amd/ops.py: the split of the samples)
# ---------------------------------------------------------------------------------------------------------------------

def kernel_instance(Lt: int) -> int:
    """KS, the template parameter (k-steps of 4 factors) the entry dispatches Lt factors to."""
    k = (Lt + 3) // 4
    return k if k <= 10 else 12 if k <= 12 else 14 if k <= 14 else 16


def host_split(E: int) -> list:
    """(samples, weight) of each call ops.poisson_nsf makes."""
    return [(min(PMAXE, E - e0), min(PMAXE, E - e0) / E) for e0 in range(0, E, PMAXE)]


def plan(N: int, D: int, Lt: int, E: int) -> dict:
    """The launch plan of a step.  With E > 32 the slice counts are those of the first (32-sample) call."""
    assert N >= 1 and D >= 1 and 1 <= Lt <= PMAXL and E >= 1
    split = host_split(E)
    ee = split[0][0]
    nblk = cdiv(N, 64)
    S = max(1, min(cdiv(1536, nblk * ee), cdiv(D, 128 * GS), 32))
    dper = cdiv(D, S)
    SN = max(1, min(cdiv(1024, cdiv(D, 64)), (N + 511) // 512, 16))
    tper = cdiv(nblk, SN)
    KS = kernel_instance(Lt)
    tail = KS % 4 == 1
    LTM = KS // 4 if tail else (KS + 3) // 4
    LP = 16 * ((KS + 3) // 4)
    EG = min(ee, PEG)
    return dict(N=N, D=D, Lt=Lt, E=E, ee=ee, split=split, nblk=nblk, S=S, dper=dper, SN=SN, tper=tper,
                empty_spot_slices=[k for k in range(SN) if k * tper >= nblk],
                empty_gene_slices=[k for k in range(S) if k * dper >= D],
                KS=KS, padded_ksteps=KS - (Lt + 3) // 4, TAIL=tail, tail_len=Lt - 16 * LTM if tail else 0, LTM=LTM,
                EG=EG, NG=cdiv(ee, EG), lds_optin=4 * 2 * (PEG * LP * 68 + 64) > 64 * 1024)


def workspace_bytes(N: int, D: int, Lt: int, E: int) -> int:
    """gpz_poisson_nsf_workspace_bytes: the pieces poisson_plan carves, each starting on a multiple of 256 bytes."""
    assert 1 <= E <= PMAXE
    p = plan(N, D, Lt, E)
    off = 0
    for count, size in ((E * Lt * N, 4),                    # exp(F)
                        (p["S"] * GS * E * Lt * N, 4),      # d exp(F) slabs, one per (gene slice, wave)
                        (p["S"] * E * GS * N, 4),           # dV slabs
                        (p["SN"] * D * Lt, 4),              # dW slabs, one per spot slice
                        (p["S"] * p["nblk"] * E, 8),        # log-lik partial sums
                        (NLG, 8)):                          # lgamma partial sums
        off = (off + 255) // 256 * 256 + count * size
    return (off + 255) // 256 * 256


def _both_sides(b: int, hi: int) -> set:
    return {x for x in (b - 1, b) if 0 <= x < hi}


def probe_genes(N: int, D: int, Lt: int, E: int) -> list:
    """The first and last gene; both sides of every gene-slice boundary k dper of pass A; next to each of those (and to
    the two ends) both sides of the neighbouring boundaries of pass B's 16-gene groups and 64-gene blocks (multiples of
    16 / 64) and of pass A's 16-gene groups (counted from the slice's first gene)."""
    p = plan(N, D, Lt, E)
    out = {0, D - 1}
    cuts = [k * p["dper"] for k in range(p["S"] + 1) if k * p["dper"] < D] + [D]
    for b in cuts:
        out |= _both_sides(b, D)
        for unit in (16, 64):
            for m in (b // unit * unit, cdiv(b, unit) * unit, (b // unit + 1) * unit, (cdiv(b, unit) - 1) * unit):
                out |= _both_sides(m, D)
    for lo, hi in zip(cuts[:-1], cuts[1:]):      # pass A: the first and the last (possibly ragged) group of the slice
        out |= _both_sides(lo + 16, hi) | _both_sides(lo + (hi - lo - 1) // 16 * 16, hi)
    return sorted(out)


def probe_spots(N: int, D: int, Lt: int, E: int) -> list:
    """The first and last spot; both sides of every spot-slice boundary k tper 64 of pass B; both sides of the last
    tile's start; the last spot of the last whole 4-spot vector group and the first of the ragged one."""
    p = plan(N, D, Lt, E)
    out = {0, N - 1}
    for k in range(1, p["SN"]):
        out |= _both_sides(k * p["tper"] * 64, N)
    out |= _both_sides((p["nblk"] - 1) * 64, N) | _both_sides(N // 4 * 4, N) | _both_sides(N // 64 * 64, N)
    return sorted(out)


def probe_positions(N: int, D: int, Lt: int, E: int) -> list:
    """(gene, spot) pairs: every probe gene and every probe spot at least once (the shorter list is cycled)."""
    g, s = probe_genes(N, D, Lt, E), probe_spots(N, D, Lt, E)
    n = max(len(g), len(s))
    return [(g[i % len(g)], s[i % len(s)]) for i in range(n)]


def probe_counts(positions: list) -> list:
    """(gene, spot, count) with the counts 1000 + (37 i mod 1000)."""
    return [(d, n, 1000 + (37 * i) % 1000) for i, (d, n) in enumerate(positions)]


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------

def _f32_exact(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(torch.float64)


def make_case(N: int, D: int, Lt: int, E: int, seed: int = 0, probes=None) -> dict:
    """fp64 CPU tensors (fp32-representable) of one problem; ``probes``: (gene, spot, count) triples written into y."""
    g = torch.Generator().manual_seed(7000 + 1009 * seed + 131 * N + 17 * D + 5 * Lt + E)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)    # noqa: E731
    c = dict(N=N, D=D, Lt=Lt, E=E, seed=seed,
             mean=0.5 * r(Lt, N), scale=0.2 + 0.5 * u(Lt, N), eps=r(E, Lt, N),
             W=0.01 + 0.3 * torch.exp(r(D, Lt)), V=torch.exp(0.7 * r(N)),
             y=torch.poisson(2.0 * u(D, N), generator=g))
    c["probes"] = list(probes or [])
    for d, n, cnt in c["probes"]:
        assert 0 <= d < D and 0 <= n < N and cnt == int(cnt) and 0 < cnt <= 20000
        c["y"][d, n] = float(cnt)
    for k, v in c.items():
        if isinstance(v, torch.Tensor):
            c[k] = _f32_exact(v)
    return c


SHARP_NEED, SHARP_AIM, COUNT_MAX = 10.0, 15.0, 20000


def required_sharpness(shape: tuple) -> tuple:
    return ("ll_lgamma", "dW") if tuple(shape) == PARTIAL_SHARPNESS else ("ll", "ll_lgamma") + OUTPUTS


_probe_cache: dict = {}


def make_probe_case(N: int, D: int, Lt: int, E: int, seed: int = 0) -> dict:
    """The case with a probe count at every probe position.  The counts start at 1000 + (37 i mod 1000); a probe whose
    share of some required output is below SHARP_AIM tolerances gets a larger count (at most 20 000), judged by the
    fp64 reference alone, until every probe meets it (tests/test_poisson_cases.py asserts SHARP_NEED = 10 on the
    result).  Without the lgamma term a probe's share of ll is y log(rate): where the rate is close to one only a large
    count makes it visible."""
    key = (N, D, Lt, E, seed)
    if key in _probe_cache:
        return _probe_cache[key]
    need = required_sharpness((N, D, Lt, E))
    probes = probe_counts(probe_positions(N, D, Lt, E))
    for _ in range(8):
        c = make_case(N, D, Lt, E, seed, probes=probes)
        nxt = []
        for (d, n, cnt), s in zip(probes, sharpness(c)):
            worst = min(s[k] for k in need)
            if worst < SHARP_AIM and cnt < COUNT_MAX:
                cnt = min(COUNT_MAX, int(cnt * min(max(1.5 * SHARP_AIM / max(worst, 1e-30), 1.5), 20.0)) + 1)
            nxt.append((d, n, cnt))
        if nxt == probes:
            break
        probes = nxt
    _probe_cache[key] = c
    return c


COUNT_VALUES = (0.0, 255.0, 256.0, 257.0, 12345.0, 2.5, 300.25)


def make_counts_case() -> dict:
    """(130, 80, 20, 3) whose y holds the values where lgamma_sum_kernel changes branch (table below 256, lgammaf from
    256 on and for non-integers), a gene row of zeros and a spot column of zeros."""
    c = make_case(130, 80, 20, 3, seed=11)
    y = c["y"]
    for i, v in enumerate(COUNT_VALUES * 6):          # scattered over rows, columns and the ragged last tile
        y[(7 * i + 3) % 80, (31 * i + 5) % 130] = v
    y[(1, 79, 40), (129, 0, 128)] = torch.tensor([12345.0, 256.0, 300.25], dtype=torch.float64)
    y[17, :] = 0.0
    y[:, 66] = 0.0
    return c


def case_key(c: dict) -> tuple:
    return (c["N"], c["D"], c["Lt"], c["E"], c["seed"], tuple(c["probes"]), float(c["y"].sum()))


# the case lists of tests/test_hip_poisson_forms.py (tests/test_poisson_cases.py asserts what they reach)
FACTOR_SWEEP = [(70, 37, Lt, 2) for Lt in range(1, PMAXL + 1)]
INSTANCE_ENDS = sorted({(128, 64, Lt, 2) for KS in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16)
                        for Lt in (min(l for l in range(1, 65) if kernel_instance(l) == KS),
                                   max(l for l in range(1, 65) if kernel_instance(l) == KS))})
EDGE_N = (1, 3, 4, 63, 64, 65, 66, 68, 127, 128, 129, 130, 192)
EDGE_D = (1, 15, 16, 17, 63, 64, 65, 149)
TILE_EDGES = [(N, 37, Lt, 3) for Lt in (20, 8) for N in EDGE_N] + [(68, D, Lt, 3) for Lt in (20, 8) for D in EDGE_D]
PLAN_CASES = [(70, 1601, 6, 2), (513, 513, 17, 9), (8193, 20, 20, 5), (64, 16385, 5, 1), (200, 149, 36, 9)] + \
             [(200, 70, 20, E) for E in (4, 8, 12, 32)]
PARTIAL_SHARPNESS = (64, 16385, 5, 1)         # one probe among 16 385 genes of a spot: sharp in ll and dW only
HOST_SPLIT = (130, 80, 20, 65)
LARGE, SMALL = (8193, 20, 20, 5), (70, 37, 20, 2)


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------

def _loglik(mean, scale, eps, W, V, y, with_lgamma):
    rate = V * torch.matmul(W, torch.exp(mean + scale * eps))          # (E,D,N)
    ll = y * torch.log(rate) - rate
    if with_lgamma:
        ll = ll - torch.lgamma(y + 1.0)
    return ll.mean(0).sum()


_ref_cache: dict = {}


def reference(c: dict, with_lgamma: bool, dtype=torch.float64) -> dict:
    """ll (python float) and dmean, dscale, dW, dV (CPU fp64 tensors) by torch autograd in ``dtype``; the fp64
    evaluation is cached per (case, with_lgamma) and shared by the tests: do not modify what it returns."""
    key = case_key(c) + (with_lgamma,)
    if dtype == torch.float64 and key in _ref_cache:
        return _ref_cache[key]
    leaf = [c[k].to(dtype).clone().requires_grad_(True) for k in ("mean", "scale", "W", "V")]
    ll = _loglik(leaf[0], leaf[1], c["eps"].to(dtype), leaf[2], leaf[3], c["y"].to(dtype), with_lgamma)
    ll.backward()
    out = dict(ll=float(ll.detach().double()))
    out.update({nm: t.grad.detach().double() for nm, t in zip(OUTPUTS, leaf)})
    if dtype == torch.float64:
        _ref_cache[key] = out
    return out


def probe_delta(c: dict, d: int, n: int, with_lgamma: bool) -> dict:
    """What the fp64 reference loses when y[d, n] alone is set to zero: ll, dW[d, :], dV[n], dmean[:, n], dscale[:, n].
    ll is a sum over (gene, spot) of terms that depend on y[d, n] only through their own entry, so the difference is
    that entry's term at its count minus its term at zero -- no approximation, and no second pass over the case
    (tests/test_poisson_cases.py compares it with the difference of two whole evaluations)."""
    leaf = [c["mean"][:, n:n + 1].clone().requires_grad_(True), c["scale"][:, n:n + 1].clone().requires_grad_(True),
            c["W"][d:d + 1].clone().requires_grad_(True), c["V"][n:n + 1].clone().requires_grad_(True)]
    y = c["y"][d:d + 1, n:n + 1]
    eps = c["eps"][:, :, n:n + 1]
    diff = _loglik(leaf[0], leaf[1], eps, leaf[2], leaf[3], y, with_lgamma) - \
        _loglik(leaf[0], leaf[1], eps, leaf[2], leaf[3], torch.zeros_like(y), with_lgamma)
    diff.backward()
    return dict(ll=float(diff.detach()), dmean=leaf[0].grad[:, 0], dscale=leaf[1].grad[:, 0], dW=leaf[2].grad[0],
                dV=leaf[3].grad[0])


def tolerance(ref: dict, name: str) -> torch.Tensor:
    """The element-wise bound the GPU test puts on an output: pytest.approx(rel=5e-5, abs=1e-3) for ll,
    assert_close(rtol=1e-3, atol=1e-3 max|ref|) for a gradient."""
    if name == "ll":
        return torch.tensor(max(LL_REL * abs(ref["ll"]), LL_ABS), dtype=torch.float64)
    r = ref[name]
    return G_ATOL * r.abs().max() + G_RTOL * r.abs()


def sharpness(c: dict, probes=None) -> list:
    """For each probe (default: the case's own) a dict with, per output, the largest |change| / tolerance over the
    entries the probe feeds; "ll" is the value without the lgamma term, "ll_lgamma" the one with it (the gradients do
    not depend on the term)."""
    ref = reference(c, False)
    tol = {k: tolerance(ref, k) for k in OUTPUTS}
    tol_ll = float(tolerance(ref, "ll"))
    tol_lg = max(LL_REL * abs(ref["ll"] - float(torch.lgamma(c["y"] + 1.0).sum())), LL_ABS)
    out = []
    for d, n, *_ in (c["probes"] if probes is None else probes):
        dl = probe_delta(c, d, n, False)
        out.append(dict(ll=abs(dl["ll"]) / tol_ll,
                        ll_lgamma=abs(dl["ll"] - float(torch.lgamma(c["y"][d, n] + 1.0))) / tol_lg,
                        dW=float((dl["dW"].abs() / tol["dW"][d]).max()),
                        dV=float(dl["dV"].abs() / tol["dV"][n]),
                        dmean=float((dl["dmean"].abs() / tol["dmean"][:, n]).max()),
                        dscale=float((dl["dscale"].abs() / tol["dscale"][:, n]).max())))
    return out
