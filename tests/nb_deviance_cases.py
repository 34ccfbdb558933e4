"""Cases, probes and the fp64 oracle for tests/test_hip_nb_deviance.py (TEST INFRASTRUCTURE ONLY; plain torch, importable
without a GPU -- tests/test_nb_deviance_cases.py checks everything here on the CPU).

The operation is gpz_nb_deviance / gpz_nb_deviance_sparse (csrc/nb_deviance.hip): under the rate mu = V W m of
tests/deviance_cases.py and one inverse dispersion theta per gene,

    dev = 2 [y log(y / mu) - (y + theta) log1p((y - mu) / (mu + theta))]    (the first term 0 at y = 0)
    ll  = lgamma(y + theta) - lgamma(theta) - lgamma(y + 1) + y log(mu / (mu + theta)) - theta log1p(mu / theta)
    pll = y log mu - mu - lgamma(y + 1)
    null model mu0 = V r_d, r_d = sum_n y / sum_n V, with the gene's own theta; 0 for a gene without counts.

The drawing, the probes, their positions and the views are those of tests/deviance_cases.py (imported, not copied); a case
here is one of its cases with ``theta`` (D,) beside it: the fp32-representable log-spaced values over [0.3, 50] across the
genes, or a per-case override.

THE REFERENCE HAS NO SUCH FUNCTION.  The oracle is fp64 torch through torch.distributions.NegativeBinomial(total_count =
theta, logits = log mu - log theta).log_prob: deviance = 2 (log_prob at mu = y, taken as 0 where y = 0, minus log_prob at mu),
the null model by the same route with mu0, and Poisson.log_prob for poisson_loglik.

Tolerances: the project's Poisson ones (tests/poisson_cases.py), scalars LL_REL |ref| + LL_ABS, vectors G_RTOL |ref| + G_ATOL
max|ref|.  A case whose plain-torch evaluation with fp32 element-wise arithmetic (the log1p form), fp64 sums and an fp64
lgamma part misses a third of any tolerance, under either value of lognormal_mean, is redrawn with the next seed: the
tolerance is never loosened."""
from __future__ import annotations

import math

import torch

import deviance_cases as DC
from deviance_cases import G_ATOL, G_RTOL, LL_ABS, LL_REL, SHARP_AIM, SHARP_NEED  # noqa: F401

SCALARS = DC.SCALARS + ("loglik", "poisson_loglik")
VECTORS = DC.VECTORS + ("loglik_per_gene", "loglik_per_spot", "poisson_loglik_per_gene")
OUTPUTS = VECTORS + SCALARS
THETA_RANGE = (0.3, 50.0)


def default_theta(D: int) -> torch.Tensor:
    lo, hi = (math.log10(v) for v in THETA_RANGE)
    return torch.logspace(lo, hi, D, dtype=torch.float64).float().double()


def with_theta(c: dict, theta=None) -> dict:
    """A copy of the case (sharing its tensors) with ``theta`` (D,): the log-spaced default, a scalar, or a (D,) tensor."""
    out = dict(c)
    D = c["y"].shape[0]
    if theta is None:
        out["theta"] = default_theta(D)
    else:
        t = torch.as_tensor(theta, dtype=torch.float64).reshape(-1)
        out["theta"] = (t.expand(D) if t.numel() == 1 else t).float().double().contiguous()
    assert out["theta"].shape == (D,) and bool((out["theta"] > 0).all())
    return out


def view(c: dict, idx) -> dict:
    return DC.view(c, idx)          # theta is per gene: the view keeps it


# ---------------------------------------------------------------------------------------------------------------------
# oracle
# ---------------------------------------------------------------------------------------------------------------------

def _nb(theta, mu):
    th = theta[:, None]
    return torch.distributions.NegativeBinomial(total_count=th, logits=torch.log(mu) - torch.log(th), validate_args=False)


def _unit_deviance(y, mu, theta):
    pos = y > 0
    sat = torch.where(pos, _nb(theta, torch.where(pos, y, torch.ones_like(y))).log_prob(y), torch.zeros_like(y))
    return 2.0 * (sat - _nb(theta, mu).log_prob(y))


def outputs_from(y, mu, V, theta) -> dict:
    dev = _unit_deviance(y, mu, theta)
    ll = _nb(theta, mu).log_prob(y)
    pll = torch.distributions.Poisson(mu, validate_args=False).log_prob(y)
    r = y.sum(1) / V.sum()
    has = (r > 0)[:, None]
    mu0 = torch.where(has, V * r[:, None], torch.ones_like(mu))
    null = torch.where(has, _unit_deviance(y, mu0, theta), torch.zeros_like(y))
    return dict(per_gene=dev.sum(1), per_spot=dev.sum(0), null_per_gene=null.sum(1), total=dev.sum(), sum_y=y.sum(),
                sum_mu=mu.sum(), null_total=null.sum(), loglik=ll.sum(), loglik_per_gene=ll.sum(1), loglik_per_spot=ll.sum(0),
                poisson_loglik=pll.sum(), poisson_loglik_per_gene=pll.sum(1))


_oracle_cache: dict = {}


def oracle(c: dict, lognormal_mean: bool = True) -> dict:
    """fp64 outputs of the case (CPU tensors); cached and shared by the tests: do not modify what it returns."""
    key = (id(c["y"]), id(c["mean"]), id(c["theta"]), bool(lognormal_mean))
    hit = _oracle_cache.get(key)
    if hit is not None and hit[0] is c["y"] and hit[1] is c["mean"] and hit[2] is c["theta"]:
        return hit[3]
    out = outputs_from(c["y"], DC.rate(c, lognormal_mean), c["V"], c["theta"])
    _oracle_cache[key] = (c["y"], c["mean"], c["theta"], out)
    return out


def _explicit_terms(y, mu, th):
    """dev, ll, pll by the formulas of the issue, in the dtype of the arguments."""
    pos = y > 0
    one = torch.ones_like(y)
    t = torch.where(pos, y * torch.log(torch.where(pos, y, one) / torch.where(pos, mu, one)), torch.zeros_like(y))
    dev = 2.0 * (t - (y + th) * torch.log1p((y - mu) / (mu + th)))
    dev = torch.where(pos, dev, 2.0 * th * torch.log1p(mu / th))
    lg1 = torch.lgamma(y + 1.0)
    ll = torch.lgamma(y + th) - torch.lgamma(th) - lg1 + y * torch.log(mu / (mu + th)) - th * torch.log1p(mu / th)
    pll = y * torch.log(mu) - mu - lg1
    return dev, ll, pll


def _sums(y, mu, dev, null, ll, pll):
    return dict(per_gene=dev.sum(1), per_spot=dev.sum(0), null_per_gene=null.sum(1), total=dev.sum(), sum_y=y.sum(),
                sum_mu=mu.sum(), null_total=null.sum(), loglik=ll.sum(), loglik_per_gene=ll.sum(1), loglik_per_spot=ll.sum(0),
                poisson_loglik=pll.sum(), poisson_loglik_per_gene=pll.sum(1))


def explicit(c: dict, lognormal_mean: bool = True) -> dict:
    """The formulas of the issue written out in fp64, without torch.distributions."""
    y, V, mu, th = c["y"], c["V"], DC.rate(c, lognormal_mean), c["theta"][:, None]
    dev, ll, pll = _explicit_terms(y, mu, th)
    r = y.sum(1) / V.sum()
    has = (r > 0)[:, None]
    null = torch.where(has, _explicit_terms(y, torch.where(has, V * r[:, None], torch.ones_like(mu)), th)[0], torch.zeros_like(y))
    return _sums(y, mu, dev, null, ll, pll)


def sparse_decomposition(c: dict, lognormal_mean: bool = True) -> dict:
    """The sums as the sparse entry splits them, in fp64: with z(mu) = theta log1p(mu / theta), a zero part over all (d, n)
    -- 2 z, -z, -mu -- plus a correction at every stored (non-zero) count."""
    y, V, mu, th = c["y"], c["V"], DC.rate(c, lognormal_mean), c["theta"][:, None]
    st = y > 0
    ys = torch.where(st, y, torch.ones_like(y))
    lg = torch.lgamma(ys + th) - torch.lgamma(th) - torch.lgamma(ys + 1.0)

    def parts(mu_):
        z = th * torch.log1p(mu_ / th)
        cd = 2.0 * (ys * torch.log(ys * (mu_ + th) / (mu_ * (ys + th))) - th * torch.log1p(ys / th))
        return z, torch.where(st, cd, torch.zeros_like(y))
    z, cd = parts(mu)
    dev = 2.0 * z + cd
    ll = -z + torch.where(st, ys * torch.log(mu / (mu + th)) + lg, torch.zeros_like(y))
    pll = -mu + torch.where(st, ys * torch.log(mu) - torch.lgamma(ys + 1.0), torch.zeros_like(y))
    r = y.sum(1) / V.sum()
    has = (r > 0)[:, None]
    z0, cd0 = parts(torch.where(has, V * r[:, None], torch.ones_like(mu)))
    null = torch.where(has, 2.0 * z0 + cd0, torch.zeros_like(y))
    return _sums(y, mu, dev, null, ll, pll)


def fp32_evaluation(c: dict, lognormal_mean: bool = True) -> dict:
    """The outputs with fp32 element-wise arithmetic (the log1p form of the deviance), fp64 sums and an fp64 lgamma part."""
    f32, f64 = torch.float32, torch.float64
    y, V, W, th = c["y"].to(f32), c["V"].to(f32), c["W"].to(f32), c["theta"].to(f32)[:, None]
    mu = V * torch.matmul(W, DC.factors(c, lognormal_mean, f32))
    pos = y > 0
    one = torch.ones_like(y)

    def unit(mu_):
        t = torch.where(pos, y * (torch.log(torch.where(pos, y, one)) - torch.log(mu_)), torch.zeros_like(y))
        d = 2.0 * (t - (y + th) * torch.log1p((y - mu_) / (mu_ + th)))
        return torch.where(pos, d, 2.0 * th * torch.log1p(mu_ / th)).to(f64)
    dev = unit(mu)
    sy = y.to(f64).sum(1)
    r = (sy / V.to(f64).sum()).to(f32)
    has = (r > 0)[:, None]
    null = torch.where(has, unit(torch.where(has, V * r[:, None], one)), torch.zeros_like(dev))
    y64, th64 = c["y"], c["theta"][:, None]
    lg1 = torch.lgamma(y64 + 1.0)
    lgp = torch.lgamma(y64 + th64) - torch.lgamma(th64)
    ll = (y * (torch.log(mu) - torch.log(th)) - (y + th) * torch.log1p(mu / th)).to(f64) + (lgp - lg1)
    pll = (y * torch.log(mu) - mu).to(f64) - lg1
    return _sums(y64, mu.to(f64), dev, null, ll, pll)


def tolerance(ref: dict, name: str) -> torch.Tensor:
    r = ref[name]
    if name in SCALARS:
        return LL_REL * r.abs() + LL_ABS
    return G_RTOL * r.abs() + G_ATOL * r.abs().max()


def figures(ref: dict, got: dict, names=OUTPUTS) -> dict:
    """Per output the largest |got - ref| / tolerance (0 where both the error and the tolerance are 0)."""
    fig = {}
    for name in names:
        g = torch.as_tensor(got[name]).detach().double().cpu()
        assert g.shape == ref[name].shape, (name, g.shape, ref[name].shape)
        err, tol = (g - ref[name]).abs(), tolerance(ref, name)
        ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)      # 0 / 0 -> 0, x / 0 -> inf
        fig[name] = float(ratio.max()) if bool(torch.isfinite(g).all()) else float("inf")
    return fig


def within_a_third(c: dict) -> bool:
    for flag in (True, False):
        if max(figures(oracle(c, flag), fp32_evaluation(c, flag)).values()) > 1.0 / 3.0:
            return False
    return True


# ---------------------------------------------------------------------------------------------------------------------
# cases: those of deviance_cases with theta; a case that misses the gate is redrawn with the next seed
# ---------------------------------------------------------------------------------------------------------------------

SEED_STEP = 100
_case_cache: dict = {}


def _first_within(build, theta, key):
    if key in _case_cache:
        return _case_cache[key]
    for attempt in range(8):
        c = with_theta(build(attempt * SEED_STEP), theta)
        if within_a_third(c):
            _case_cache[key] = c
            return c
    raise AssertionError(f"no draw of {key} keeps the fp32 evaluation within a third of the tolerances")


def _tkey(theta):
    return None if theta is None else tuple(torch.as_tensor(theta, dtype=torch.float64).reshape(-1).tolist())


def make_case(N, D, Lt, seed=0, probes=None, density=1.0, edit=None, theta=None) -> dict:
    return _first_within(lambda s: DC.make_case(N, D, Lt, seed + s, probes, density, edit), theta,
                         ("case", N, D, Lt, seed, tuple(probes or ()), density, edit, _tkey(theta)))


PROBE_WORTH = 500.0


def _grown(N, D, Lt, positions, seed, density, edit, theta):
    """A probe at every position, the counts chosen for the NB outputs.  The counts deviance_cases grows (1000 and up, the
    same for every gene) are sharp in the Poisson deviance and not in this one: under a small theta the unit NB deviance of
    an outlier grows like 2 theta y / mu only, while the tolerances' max|ref| term follows the probes of the genes with a
    large theta.  So the counts are balanced instead: every probe gets the smallest count (of a ladder of half-octaves up
    to COUNT_MAX, above twice its rate) whose unit deviance differs from that of a zero count by the same worth -- PROBE_WORTH,
    or what the weakest probe reaches at COUNT_MAX.  A probe is then about 1 / (number of probes of its gene + 1) of the
    largest per-gene sum, hundreds of tolerances; tests/test_nb_deviance_cases.py asserts SHARP_NEED by the oracle."""
    base = with_theta(DC.make_case(N, D, Lt, seed, None, density, edit), theta)
    d = torch.tensor([p[0] for p in positions])
    n = torch.tensor([p[1] for p in positions])
    mu, th = DC.rate(base, True)[d, n][:, None], base["theta"][d][:, None]
    steps = int(2 * math.log2(DC.COUNT_MAX / 8.0))
    ladder = torch.unique(torch.cat([torch.round(8.0 * 2.0 ** (0.5 * torch.arange(steps + 1, dtype=torch.float64))),
                                     torch.tensor([float(DC.COUNT_MAX)], dtype=torch.float64)]))
    y = ladder[None, :].expand(len(positions), -1)
    worth = (_explicit_terms(y, mu.expand_as(y), th.expand_as(y))[0] - 2.0 * th * torch.log1p(mu / th)).abs()
    worth = torch.where(y >= 2.0 * mu + 8.0, worth, torch.zeros_like(worth))
    aim = min(PROBE_WORTH, float(worth[:, -1].min()))
    first = (worth >= aim).double().argmax(dim=1)
    probes = [(int(d[i]), int(n[i]), int(ladder[first[i]])) for i in range(len(positions))]
    return with_theta(DC.make_case(N, D, Lt, seed, probes, density, edit), theta)


def make_probe_case(N, D, Lt, positions, seed=0, density=1.0, edit=None, theta=None) -> dict:
    return _first_within(lambda s: _grown(N, D, Lt, positions, seed + s, density, edit, theta), theta,
                         ("probe", N, D, Lt, tuple(positions), seed, density, edit, _tkey(theta)))


def dense_case(N, D, Lt, plan, seed=0, theta=None) -> dict:
    """deviance_cases.dense_case (probes at every boundary ``plan`` reports; the exact one-spot case for N = 1) with theta."""
    if N == 1:
        return _first_within(lambda s: DC.one_spot_case(D, Lt, seed + s), theta, ("one", D, Lt, seed, _tkey(theta)))
    return make_probe_case(N, D, Lt, DC.dense_positions(N, D, plan), seed, theta=theta)


def zeros_cases() -> dict:
    return dict(all_zero=make_case(130, 80, 5, seed=3, edit=_all_zero),
                empty_gene_and_spot=make_probe_case(130, 80, 5, [(0, 0), (0, 129), (79, 0), (79, 129), (16, 65), (18, 67)],
                                                    seed=4, edit=DC._empty_gene_and_spot))


def _all_zero(y):
    y.zero_()


def chunk_case(chunk: int, Lt: int = 5, theta=None) -> dict:
    """deviance_cases.chunk_case -- its shape, its rows of one chunk, one chunk + 1 and three chunks of non-zeros, its probe
    positions -- with the probe counts grown for the NB outputs."""
    base = DC.chunk_case(chunk, Lt)
    lens = base["row_lengths"]

    def edit(y):
        for d, n in lens.items():
            y[d, :n] = y[d, :n].clamp(min=1.0)
            y[d, n:] = 0.0
    c = make_probe_case(base["N"], base["D"], Lt, sorted((d, n) for d, n, _ in base["probes"]), seed=5, density=0.05,
                        edit=DC._Edit(edit, ("nb-chunk", chunk)), theta=theta)
    c["row_lengths"] = lens
    return c


def view_case() -> tuple:
    """(case with N = 130 spots, idx) of deviance_cases.view_case: its unsorted idx of 37 spots and its probe positions."""
    idx = DC.view_case()[1]
    return make_probe_case(130, 80, 5, DC.VIEW_PROBES, seed=6, density=0.3), idx


# theta extremes (the GPU tests' mid-size shape)
MID = (130, 80, 20)
THETA_SMALL, THETA_LARGE, THETA_LIMIT = 0.05, 1e6, 1e7


def mixed_theta(D: int, tile: int) -> torch.Tensor:
    """Every wave tile of ``tile`` genes holds the whole range: 0.3 ... 1e6 log-spaced within the tile."""
    lo, hi = math.log10(THETA_RANGE[0]), math.log10(THETA_LARGE)
    within = torch.logspace(lo, hi, tile, dtype=torch.float64)
    return within.repeat(-(-D // tile))[:D].float().double()


def limit_case() -> dict:
    """A probe-free case at theta = 1e7: the NB deviance and log density are the Poisson ones to within the tolerances."""
    return make_case(*MID, seed=11, theta=THETA_LIMIT)


# ---------------------------------------------------------------------------------------------------------------------
# probes
# ---------------------------------------------------------------------------------------------------------------------

ONE_THETA_OUTPUTS = ("null_total", "null_per_gene", "poisson_loglik", "poisson_loglik_per_gene")


def fully_probed(c: dict) -> bool:
    """Whether one count can be sharp in all eleven outputs it feeds.  With theta spread over [0.3, 50] across the genes it
    cannot, whatever the counts: (a) the NB deviance is robust to an outlier by construction -- under a small theta one
    count moves the null deviance of its gene by a few theta log 2 per spot, while the tolerance G_ATOL max|ref| follows
    the genes with a large theta; (b) a count large enough to show in the NB outputs of a gene with a small theta
    (2 theta y / mu) is worth y log(y / mu), a hundred times as much, in the Poisson log density, whose max|ref| then hides
    the moderate counts that the genes with a large theta need.  So in those cases a probe is judged by the seven outputs of
    the NB deviance, the NB log density and sum_y; the null deviance and the Poisson log density are judged, with all the
    others, in the cases whose theta is THETA_LARGE for every gene -- the mid-size, the sliced and the chunk case have such
    a twin -- and are held to the tolerances everywhere."""
    return float(c["theta"].min()) >= THETA_LARGE


def sharpness(c: dict, lognormal_mean: bool = True, probes=None) -> list:
    """Per probe the smallest |change| / tolerance over the outputs it feeds when its count alone is set to zero: the six
    of the Poisson cases, loglik and poisson_loglik, loglik_per_gene and poisson_loglik_per_gene at its gene, and
    loglik_per_spot at its spot (without ONE_THETA_OUTPUTS unless the case is ``fully_probed``)."""
    ref, mu = oracle(c, lognormal_mean), DC.rate(c, lognormal_mean)
    skip = () if fully_probed(c) else ONE_THETA_OUTPUTS
    out = []
    for d, n, *_ in (c["probes"] if probes is None else probes):
        y = c["y"].clone()
        y[d, n] = 0.0
        alt = outputs_from(y, mu, c["V"], c["theta"])
        worst = []
        for name in ("total", "sum_y", "null_total", "loglik", "poisson_loglik"):
            if name not in skip:
                worst.append(float((alt[name] - ref[name]).abs() / tolerance(ref, name)))
        for name, i in (("per_gene", d), ("null_per_gene", d), ("per_spot", n), ("loglik_per_gene", d),
                        ("poisson_loglik_per_gene", d), ("loglik_per_spot", n)):
            if name not in skip:
                worst.append(float((alt[name][i] - ref[name][i]).abs() / tolerance(ref, name)[i]))
        out.append(min(worst))
    return out
