"""Case builders, probes and the fp64 oracle for tests/test_hip_deviance.py (TEST INFRASTRUCTURE ONLY; plain torch,
importable without a GPU -- tests/test_deviance_cases.py checks everything here on the CPU).

The operation is the Poisson deviance under the predictive mean rate, gpz_poisson_deviance / gpz_poisson_deviance_sparse
(csrc/deviance.hip):

    m = exp(mean + scale^2 / 2)   (exp(mean) without lognormal_mean),   mu = V W m,
    dev = 2 (y log(y / mu) - y + mu), the log term 0 at y = 0;   per_gene, per_spot, total, sum_y, sum_mu,
    null model mu0 = V r_d, r_d = sum_n y / sum_n V:   null_per_gene, null_total.

THE REFERENCE HAS NO DEVIANCE FUNCTION (its anndata_to_train_val prepares a validation set that nothing scores), so there
is no reference run to pin these outputs to.  The oracle is fp64 torch on the same fp32-representable inputs, through
torch.distributions.Poisson: dev = 2 (log_prob(y | y) - log_prob(y | mu)) (the lgamma terms cancel; torch's xlogy makes
the log term 0 at y = 0), and the same route with mu0 for the null model.

Tolerances: the project's Poisson ones (tests/poisson_cases.py).  Scalars |got - ref| <= LL_REL |ref| + LL_ABS; per_gene,
per_spot, null_per_gene G_RTOL |ref| + G_ATOL max|ref|.  ``make_case`` verifies for every case that a plain torch evaluation
with fp32 element-wise arithmetic and fp64 sums stays within a third of every tolerance against the oracle and redraws the
case (next seed) otherwise: the tolerance is never loosened.

A *probe* is one large integer count at an element that a wrong bound of a tile, slice or chunk would drop or count twice:
the corners of the matrix and the first and last element of every tile and chunk the plan queries report (no boundary is
restated here).  Probe counts are grown until each is worth at least SHARP_AIM tolerances in every output it feeds (total,
sum_y, null_total, its gene's per_gene and null_per_gene, its spot's per_spot), judged by the oracle alone;
tests/test_deviance_cases.py asserts SHARP_NEED."""
from __future__ import annotations

import torch

from poisson_cases import COUNT_MAX, G_ATOL, G_RTOL, LL_ABS, LL_REL, SHARP_AIM, SHARP_NEED  # noqa: F401

SCALARS = ("total", "sum_y", "sum_mu", "null_total")
VECTORS = ("per_gene", "per_spot", "null_per_gene")
OUTPUTS = VECTORS + SCALARS


def _f32_exact(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(torch.float64)


# ---------------------------------------------------------------------------------------------------------------------
# oracle
# ---------------------------------------------------------------------------------------------------------------------

def factors(c: dict, lognormal_mean: bool, dtype=torch.float64) -> torch.Tensor:
    mean, scale = c["mean"].to(dtype), c["scale"].to(dtype)
    return torch.exp(mean + 0.5 * scale * scale) if lognormal_mean else torch.exp(mean)


def rate(c: dict, lognormal_mean: bool) -> torch.Tensor:
    return c["V"] * torch.matmul(c["W"], factors(c, lognormal_mean))


def _unit_deviance(y, mu):
    P = torch.distributions.Poisson
    return 2.0 * (P(y, validate_args=False).log_prob(y) - P(mu, validate_args=False).log_prob(y))


def outputs_from(y, mu, V) -> dict:
    """Every output from the counts, the rate and the size factors, in their dtype, by the torch.distributions route."""
    dev = _unit_deviance(y, mu)
    r = y.sum(1) / V.sum()
    null = _unit_deviance(y, V * r[:, None])
    return dict(per_gene=dev.sum(1), per_spot=dev.sum(0), null_per_gene=null.sum(1), total=dev.sum(), sum_y=y.sum(),
                sum_mu=mu.sum(), null_total=null.sum())


def view(c: dict, idx) -> dict:
    """The case restricted to the spots idx (a 1-D int64 tensor), in idx's order."""
    out = dict(c)
    for k in ("mean", "scale", "y"):
        out[k] = c[k][:, idx]
    out["V"] = c["V"][idx]
    out["N"] = int(idx.numel())
    return out


_oracle_cache: dict = {}


def oracle(c: dict, lognormal_mean: bool = True) -> dict:
    """fp64 outputs of the case (CPU tensors); cached and shared by the tests: do not modify what it returns."""
    key = (id(c["y"]), id(c["mean"]), bool(lognormal_mean))
    hit = _oracle_cache.get(key)
    if hit is not None and hit[0] is c["y"] and hit[1] is c["mean"]:
        return hit[2]
    out = outputs_from(c["y"], rate(c, lognormal_mean), c["V"])
    _oracle_cache[key] = (c["y"], c["mean"], out)
    return out


def explicit(c: dict, lognormal_mean: bool = True) -> dict:
    """The formulas of the issue written out, without torch.distributions."""
    y, V, mu = c["y"], c["V"], rate(c, lognormal_mean)

    def unit(mu_):
        safe = torch.where(y > 0, mu_, torch.ones_like(mu_))
        t = torch.where(y > 0, y * torch.log(torch.where(y > 0, y, torch.ones_like(y)) / safe), torch.zeros_like(y))
        return 2.0 * (t - y + mu_)
    dev = unit(mu)
    null = unit(V * (y.sum(1) / V.sum())[:, None])
    return dict(per_gene=dev.sum(1), per_spot=dev.sum(0), null_per_gene=null.sum(1), total=dev.sum(), sum_y=y.sum(),
                sum_mu=mu.sum(), null_total=null.sum())


def factorised_sum_mu(c: dict, lognormal_mean: bool = True) -> dict:
    """sum mu the way the sparse entry forms it: per gene W a, a = m V; per spot V (c . m), c = column sums of W."""
    m = factors(c, lognormal_mean)
    return dict(per_gene=torch.matmul(c["W"], torch.matmul(m, c["V"])), per_spot=c["V"] * torch.matmul(c["W"].sum(0), m))


def fp32_evaluation(c: dict, lognormal_mean: bool = True) -> dict:
    """The outputs with fp32 element-wise arithmetic and fp64 sums, by the route a kernel takes: y log(y / mu) from the two
    logarithms, the null deviance from the per-gene sums of y, y log y and y log V."""
    f32, f64 = torch.float32, torch.float64
    y, V, W = c["y"].to(f32), c["V"].to(f32), c["W"].to(f32)
    mu = V * torch.matmul(W, factors(c, lognormal_mean, f32))
    ly = torch.log(torch.where(y > 0, y, torch.ones_like(y)))
    t = torch.where(y > 0, y * (ly - torch.log(mu)), torch.zeros_like(y))
    dev = (2.0 * ((t - y) + mu)).to(f64)
    sy, syly, sylv = y.to(f64).sum(1), (y * ly).to(f64).sum(1), (y * torch.log(V)).to(f64).sum(1)
    pos = sy > 0
    r = torch.where(pos, sy, torch.ones_like(sy)) / V.to(f64).sum()
    null = torch.where(pos, 2.0 * (syly - sylv - sy * torch.log(r)), torch.zeros_like(sy))
    return dict(per_gene=dev.sum(1), per_spot=dev.sum(0), null_per_gene=null, total=dev.sum(), sum_y=sy.sum(),
                sum_mu=mu.to(f64).sum(), null_total=null.sum())


def tolerance(ref: dict, name: str) -> torch.Tensor:
    r = ref[name]
    if name in SCALARS:
        return LL_REL * r.abs() + LL_ABS
    return G_RTOL * r.abs() + G_ATOL * r.abs().max()


def figures(ref: dict, got: dict) -> dict:
    """Per output the largest |got - ref| / tolerance (0 where both the error and the tolerance are 0)."""
    fig = {}
    for name in OUTPUTS:
        g = torch.as_tensor(got[name]).detach().double().cpu()
        assert g.shape == ref[name].shape, (name, g.shape, ref[name].shape)
        err, tol = (g - ref[name]).abs(), tolerance(ref, name)
        ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)      # 0 / 0 -> 0, x / 0 -> inf
        fig[name] = float(ratio.max()) if bool(torch.isfinite(g).all()) else float("inf")
    return fig


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------

def _draw(N: int, D: int, Lt: int, seed: int, density: float) -> dict:
    g = torch.Generator().manual_seed(9000 + 1009 * seed + 131 * N + 17 * D + 5 * Lt)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)    # noqa: E731
    c = dict(N=N, D=D, Lt=Lt, seed=seed, mean=0.5 * r(Lt, N), scale=0.2 + 0.5 * u(Lt, N),
             W=0.01 + 0.3 * torch.exp(r(D, Lt)), V=torch.exp(0.7 * r(N)), y=torch.poisson(2.0 * u(D, N), generator=g))
    if density < 1.0:
        c["y"] = c["y"] * (u(D, N) < density)
    return c


def within_a_third(c: dict) -> bool:
    for flag in (True, False):
        fig = figures(oracle(c, flag), fp32_evaluation(c, flag))
        if max(fig.values()) > 1.0 / 3.0:
            return False
    return True


def make_case(N: int, D: int, Lt: int, seed: int = 0, probes=None, density: float = 1.0, edit=None) -> dict:
    """fp64 CPU tensors (fp32-representable) of one problem.  ``probes``: (gene, spot, count) triples written into y;
    ``edit``: a function applied to y before the probes (structure such as empty rows).  Redrawn with the next seed until
    the fp32 evaluation stays within a third of every tolerance."""
    for attempt in range(8):
        c = _draw(N, D, Lt, seed + 1000 * attempt, density)
        if edit is not None:
            edit(c["y"])
        c["probes"] = list(probes or [])
        for d, n, cnt in c["probes"]:
            assert 0 <= d < D and 0 <= n < N and cnt == int(cnt) and 0 < cnt <= COUNT_MAX
            c["y"][d, n] = float(cnt)
        for k, v in c.items():
            if isinstance(v, torch.Tensor):
                c[k] = _f32_exact(v)
        if within_a_third(c):
            return c
    raise AssertionError(f"no draw of {(N, D, Lt, seed)} keeps the fp32 evaluation within a third of the tolerances")


def sharpness(c: dict, lognormal_mean: bool = True, probes=None) -> list:
    """Per probe the smallest |change| / tolerance over the outputs it feeds when its count alone is set to zero."""
    ref, mu = oracle(c, lognormal_mean), rate(c, lognormal_mean)
    out = []
    for d, n, *_ in (c["probes"] if probes is None else probes):
        y = c["y"].clone()
        y[d, n] = 0.0
        alt = outputs_from(y, mu, c["V"])
        worst = []
        for name in ("total", "sum_y", "null_total"):
            worst.append(float((alt[name] - ref[name]).abs() / tolerance(ref, name)))
        for name, i in (("per_gene", d), ("null_per_gene", d), ("per_spot", n)):
            worst.append(float((alt[name][i] - ref[name][i]).abs() / tolerance(ref, name)[i]))
        out.append(min(worst))
    return out


_case_cache: dict = {}


def make_probe_case(N: int, D: int, Lt: int, positions, seed: int = 0, density: float = 1.0, edit=None) -> dict:
    """The case with a probe at every (gene, spot) of ``positions``; counts 1000 + (37 i mod 1000), grown (at most to
    COUNT_MAX) until every probe is worth SHARP_AIM tolerances under both values of lognormal_mean."""
    key = (N, D, Lt, tuple(positions), seed, density, edit)
    if key in _case_cache:
        return _case_cache[key]
    probes = [(d, n, 1000 + (37 * i) % 1000) for i, (d, n) in enumerate(positions)]
    for _ in range(6):
        c = make_case(N, D, Lt, seed, probes, density, edit)
        s = [min(a, b) for a, b in zip(sharpness(c, True), sharpness(c, False))]
        nxt = [(d, n, min(COUNT_MAX, 2 * cnt) if w < SHARP_AIM else cnt) for (d, n, cnt), w in zip(probes, s)]
        if nxt == probes:
            break
        probes = nxt
    _case_cache[key] = c
    return c


def _sides(b: int, hi: int) -> set:
    return {x for x in (b - 1, b) if 0 <= x < hi}


def _pairs(genes, spots) -> list:
    g, s = sorted(genes), sorted(spots)
    n = max(len(g), len(s))
    return sorted({(g[i % len(g)], s[i % len(s)]) for i in range(n)} | {(g[0], s[0]), (g[0], s[-1]), (g[-1], s[0]), (g[-1], s[-1])})


def dense_positions(N: int, D: int, plan: dict) -> list:
    """The four corners, and every gene / spot on either side of a boundary ``plan`` (ops.poisson_deviance_plan) reports:
    the wave tiles (genes_per_tile, spots_per_tile), the workgroups' gene blocks, the spot slices, and the last whole
    4-spot vector group of a row."""
    genes, spots = {0, D - 1}, {0, N - 1}
    for unit in (plan["genes_per_tile"], plan["genes_per_block"]):
        for b in range(unit, D, unit):
            genes |= _sides(b, D)
    ts = plan["spots_per_tile"]
    for b in range(ts, N, ts):
        spots |= _sides(b, N)
    for k in range(1, plan["spot_slices"]):
        spots |= _sides(k * plan["tiles_per_spot_slice"] * ts, N)
    spots |= _sides(N // 4 * 4, N)
    return _pairs(genes, spots)


# shapes of the GPU tests; an edge is (multiple of the plan's unit, offset)
FACTOR_COUNTS = (1, 4, 5, 20, 63, 64)
EDGE_SPOTS = ((0, 1), (1, -1), (1, 0), (1, 1), (2, 1), (0, 3), (1, 2))             # of spots_per_tile: 1, 63, 64, 65, 129, 3, 66
EDGE_GENES = ((0, 1), (1, -1), (1, 0), (1, 1))                                     # of genes_per_tile: 1, 15, 16, 17
EDGE_BLOCKS = ((1, -1), (1, 0), (1, 1), (2, -1), (2, 0), (2, 1))                   # of genes_per_block: 63 .. 129
ONE_SPOT_GENES = 17                                                                # genes of the N = 1 case
SLICED = (1100, 20, 5)                                                             # more than one spot slice


def edge(unit: int, e: tuple) -> int:
    return e[0] * unit + e[1]


def one_spot_case(D: int, Lt: int, seed: int = 0) -> dict:
    """N = 1.  With one spot the null model reproduces the counts (V r_d = y), its deviance is identically zero and so is
    the tolerance G_RTOL |ref| + G_ATOL max|ref| of null_per_gene: only an evaluation that is exact passes.  The three-sum
    route (sum y log y - sum y log V - Sy log r) is exact in fp32 as in fp64 when every logarithm in it is, i.e. for counts
    in {0, 1} and V = 1; with any larger count it is rounding noise of the size y log y * 2^-24 in fp32 (and 2^-53 in the
    fp64 oracle itself), which no draw brings under a tolerance of zero.  So this case has such counts and no large
    probes; the factors are shifted so that mu is far from y, and per_gene[d] IS the unit deviance of its one element:
    a dropped or doubled element moves it by its whole value; the case is redrawn until that is SHARP_AIM tolerances of
    per_spot[0], the sum of them all, too (tests/test_deviance_cases.py asserts SHARP_NEED)."""
    def edit(y):
        y.clamp_(max=1.0)
    for attempt in range(8):
        c = _draw(1, D, Lt, seed + 1000 * attempt, 1.0)
        edit(c["y"])
        c["mean"] = c["mean"] + 2.5
        c["V"] = torch.ones(1, dtype=torch.float64)
        c["probes"] = []
        for k, v in c.items():
            if isinstance(v, torch.Tensor):
                c[k] = _f32_exact(v)
        sharp = all(float((oracle(c, f)["per_gene"] / tolerance(oracle(c, f), "per_spot")[0]).min()) >= SHARP_AIM for f in (True, False))
        if within_a_third(c) and sharp:
            return c
    raise AssertionError("no one-spot draw keeps the fp32 evaluation within a third of the tolerances")


def dense_case(N: int, D: int, Lt: int, plan: dict, seed: int = 0) -> dict:
    if N == 1:
        return one_spot_case(D, Lt, seed)
    return make_probe_case(N, D, Lt, dense_positions(N, D, plan), seed)


def _empty_gene_and_spot(y):
    y[17, :] = 0.0
    y[:, 66] = 0.0


def zeros_cases() -> dict:
    """An all-zero y, and one gene (17) and one spot (66) without counts inside an otherwise filled matrix."""
    return dict(all_zero=make_case(130, 80, 5, seed=3, edit=lambda y: y.zero_()),
                empty_gene_and_spot=make_probe_case(130, 80, 5, [(0, 0), (0, 129), (79, 0), (79, 129), (16, 65), (18, 67)],
                                                    seed=4, edit=_empty_gene_and_spot))


def chunk_case(chunk: int, Lt: int = 5) -> dict:
    """Sparse: gene rows of exactly one chunk, one chunk + 1 and three chunks of non-zeros (``chunk`` from
    ops.poisson_deviance_sparse_plan), the rest about 5 % filled; probes at the first and last entry of every chunk of
    those rows and at the corners."""
    N, D = 3 * chunk + 64, 6
    lens = {1: chunk, 2: chunk + 1, 3: 3 * chunk}

    def edit(y):
        for d, n in lens.items():
            y[d, :n] = y[d, :n].clamp(min=1.0)       # stored
            y[d, n:] = 0.0
    pos = {(0, 0), (0, N - 1), (D - 1, 0), (D - 1, N - 1)}
    for d, n in lens.items():
        for b in list(range(0, n, chunk)) + [n]:
            pos |= {(d, x) for x in _sides(b, n)}
    c = make_probe_case(N, D, Lt, sorted(pos), seed=5, density=0.05, edit=_Edit(edit, ("chunk", chunk)))
    c["row_lengths"] = lens
    return c


class _Edit:
    """A y edit with a hashable identity (the case cache's key)."""

    def __init__(self, fn, key):
        self.fn, self.key = fn, key

    def __call__(self, y):
        self.fn(y)

    def __hash__(self):
        return hash(self.key)

    def __eq__(self, other):
        return isinstance(other, _Edit) and self.key == other.key


VIEW_PROBES = [(0, 0), (79, 129), (40, 64), (15, 63), (16, 70), (33, 5)]
VIEW_EXCLUDED_PROBE = (40, 64)


def view_case() -> tuple:
    """(case with N = 130 spots, idx): an unsorted idx of 37 spots that holds the first and the last spot and every probe
    spot but 64, which carries the probe (40, 64)."""
    c = make_probe_case(130, 80, 5, VIEW_PROBES, seed=6, density=0.3)
    g = torch.Generator().manual_seed(61)
    must = [129, 0, 63, 70, 5]
    rest = [n for n in torch.randperm(130, generator=g).tolist() if n not in must and n != VIEW_EXCLUDED_PROBE[1]]
    idx = torch.tensor(must + rest[:37 - len(must)], dtype=torch.int64)
    idx = idx[torch.randperm(37, generator=g)]
    assert idx.numel() == 37 and len(set(idx.tolist())) == 37 and bool((idx[1:] < idx[:-1]).any())
    return c, idx
