"""Cases, classification and bounds for tests/test_hip_count_range.py (TEST INFRASTRUCTURE ONLY; plain torch and numpy,
importable without a GPU -- tests/test_range_cases.py checks everything here on the CPU).

The eight fused entries that score counts -- the Poisson and negative-binomial steps and deviances, dense and sparse -- are
covered for shape elsewhere; every case there draws rates of 0.3 .. 2 and theta in [0.3, 50].  The cases here walk the VALUE
range instead: rate levels 1e-6 .. 1e4, theta 1e-2 .. 1e6, a narrow and a wide (ten decades inside one tile) latent spread,
and one mixed case whose 16-gene tiles each hold eight regimes.

Oracles and tolerances are those of the existing case modules (nb_cases.oracle, poisson_cases.reference,
deviance_cases.oracle, nb_deviance_cases.oracle; LL_REL, LL_ABS, G_RTOL, G_ATOL), imported, not restated.  What is new:

  * dtheta is bounded by G_RTOL |ref| + G_ATOL C_d with C_d the sum of the absolute values of dtheta's summands
    (``theta_cancel``): near the Poisson limit dtheta's terms cancel to O(1 / theta^2), and the bound of
    test_hip_nb.py::test_near_poisson_limit is this one without the sample-dependent terms;
  * in the mixed case the per-gene outputs take max|ref| over the genes of the same regime, not over the whole output, so a
    gene at rate 1e-3 is not hidden behind one at rate 1e2;
  * the value with the lgamma(y + 1) term is bounded by LL_REL (|value without it| + sum lgamma(y + 1)) + LL_ABS: the two
    parts cancel at large counts.

Classification, by the oracle side alone: for every (case, family, output) the figure -- largest error / bound -- of a plain
evaluation with fp32 element-wise arithmetic and fp64 sums (the theta-only lgamma and digamma terms in fp64, as the kernels
have them).  An output is *in domain* when that figure is at most 1/3, the rule of deviance_cases.make_case.  ``floor`` names
the outputs that must be in domain; a case that misses its floor is redrawn with the next seed, never moved out of the floor,
and no tolerance is touched.  Three deviance sums at rates of 1e4 are out of domain for the plain evaluation at every seed
(``F32_SHORT``, with the reason); they stay in the floor for the kernels, which ``allowed`` holds to the plain bound there.
Out of domain (fp32 cancellation in y / Z - V (y + theta) / (mu + theta) at mu / theta >= 1e4, and in y (log y - log mu) at
counts of 1e4) a kernel is held to max(bound, 4 x the error of that evaluation), element-wise."""
from __future__ import annotations

import numpy as np
import torch

import deviance_cases as DC
import nb_cases as NB
import nb_deviance_cases as NDC
import poisson_cases as PC
from poisson_cases import G_ATOL, G_RTOL, LL_ABS, LL_REL

D, N, LT, E = 33, 130, 5, 3               # two ragged 16-gene groups, two 64-spot tiles + 2 spots, N % 4 != 0
SPREAD = {"narrow": (0.3, 0.3), "wide": (3.0, 1.5)}          # mean = a randn, scale = 0.2 + b rand
LEVELS = (1e-6, 1e-3, 1.0, 1e2)
THETAS = (1e-2, 1.0, 1e2, 1e4, 1e6)
LARGE_LEVEL, LARGE_THETAS = 1e4, (1e2, 1e4, 1e6)
NB_GRID = [(lv, th, "narrow") for lv in LEVELS for th in THETAS] + \
          [(lv, th, "wide") for lv in LEVELS if lv <= 1 for th in THETAS] + \
          [(LARGE_LEVEL, th, "narrow") for th in LARGE_THETAS]
POISSON_THETA = 1e2                       # the Poisson entries read no theta: their cases are the NB cases at this one
POISSON_GRID = [(lv, POISSON_THETA, sp) for lv, th, sp in NB_GRID if th == POISSON_THETA]
MIXED_D = 40
REG = [(1e-6, 1.0), (1e-3, 1e2), (1e-3, 1e6), (1.0, 1.0), (1.0, 1e2), (1.0, 1e4), (1e2, 1e2), (1e2, 1e4)]   # (level, theta)
IN_DOMAIN = 1.0 / 3.0
OUT_OF_DOMAIN_MARGIN = 4.0                # test_hip_nmf.py's margin over the reference's own fp32 noise

FAMILIES = ("poisson_step", "nb_step", "poisson_deviance", "nb_deviance")
STEP_GRADS = ("dmean", "dscale", "dW", "dV")
OUTPUTS = {"poisson_step": ("ll", "ll_lgamma") + STEP_GRADS, "nb_step": ("ll", "ll_lgamma") + STEP_GRADS + ("dtheta",),
           "poisson_deviance": DC.OUTPUTS, "nb_deviance": NDC.OUTPUTS}
PER_GENE = ("dW", "dtheta", "per_gene", "null_per_gene", "loglik_per_gene", "poisson_loglik_per_gene")


def _f32_exact(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(torch.float64)


def mean_rate(c: dict) -> torch.Tensor:
    """V W exp(mean + scale^2 / 2) (D, N): the rate the counts are drawn from and the deviances score."""
    return DC.rate(c, True)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------

def _build(levels: torch.Tensor, thetas: torch.Tensor, spread: str, seed: int, V=None) -> dict:
    """One problem, fp64 tensors of fp32-representable values.  ``levels`` with one entry: W is rescaled as a whole so the
    median rate is that level; with one entry per gene: every row of W to its own."""
    Dg = int(thetas.numel())
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)    # noqa: E731
    a, b = SPREAD[spread]
    c = dict(N=N, D=Dg, Lt=LT, E=E, seed=seed, spread=spread, probes=[],
             mean=_f32_exact(a * r(LT, N)), scale=_f32_exact(0.2 + b * u(LT, N)), eps=_f32_exact(r(E, LT, N)),
             W=u(Dg, LT) + 0.05, V=_f32_exact(torch.exp(0.7 * r(N)) if V is None else V(g)), theta=_f32_exact(thetas))
    mu = mean_rate(c)
    med = mu.median() if levels.numel() == 1 else mu.median(dim=1, keepdim=True).values
    c["W"] = _f32_exact(c["W"] * (levels.reshape(-1, 1) / med))
    c["levels"] = levels.expand(Dg).clone()
    mu = mean_rate(c).numpy()
    shape = c["theta"].numpy()[:, None]
    rng = np.random.default_rng(seed)                  # gamma-Poisson as nb_cases.make_inputs draws it
    c["y"] = torch.from_numpy(rng.poisson(rng.gamma(shape, mu / shape)).astype(np.float64))
    c["yp"] = torch.from_numpy(np.random.default_rng([seed, 1]).poisson(mu).astype(np.float64))
    for k in ("y", "yp"):
        assert float(c[k].max()) < 2 ** 24 and bool((_f32_exact(c[k]) == c[k]).all()), k
    return c


_cases: dict = {}


def _first_in_floor(key, build, seed):
    """The first of the seeds seed, seed + 1, ... whose case meets its floor (the tolerances stay)."""
    if key not in _cases:
        for attempt in range(8):
            c = build(seed + attempt)
            if all(not missed_floor(c, fam) for fam in families_of(c)):
                break
        else:
            raise AssertionError(f"no draw of {key} keeps the floor's outputs within a third of their bounds")
        _cases[key] = c
    return _cases[key]


def regime_case(level: float, theta: float, spread: str, seed=None) -> dict:
    """One regime for all genes: median rate ``level``, the same ``theta`` for every gene."""
    if seed is None:
        seed = 5000 + 16 * NB_GRID.index((level, theta, spread))

    def build(s):
        c = _build(torch.tensor([level], dtype=torch.float64), torch.full((D,), theta, dtype=torch.float64), spread, s)
        c.update(kind="regime", level=level, theta_all=theta, blocks=None, poisson_blocks=None)
        return c
    return _first_in_floor((level, theta, spread, seed), build, seed)


def mixed_case(seed: int = 7000) -> dict:
    """Gene d in regime REG[d % 8], so every 16-gene tile holds all eight; V log-spaced over 1e-2 .. 1e2, permuted."""
    blocks = torch.arange(MIXED_D) % len(REG)
    levels = torch.tensor([REG[int(b)][0] for b in blocks], dtype=torch.float64)
    thetas = torch.tensor([REG[int(b)][1] for b in blocks], dtype=torch.float64)
    lv = sorted({lvl for lvl, _ in REG})

    def build(s):
        c = _build(levels, thetas, "narrow", s,
                   V=lambda g: torch.logspace(-2, 2, N, dtype=torch.float64)[torch.randperm(N, generator=g)])
        c.update(kind="mixed", level=None, theta_all=None, blocks=blocks,
                 poisson_blocks=torch.tensor([lv.index(float(x)) for x in levels]))     # the Poisson entries: levels only
        return c
    return _first_in_floor(("mixed", seed), build, seed)


def families_of(c: dict) -> tuple:
    """The families a case serves: the Poisson entries take the mixed case and the regime cases of POISSON_GRID."""
    if c["kind"] == "mixed" or c["theta_all"] == POISSON_THETA:
        return FAMILIES
    return ("nb_step", "nb_deviance")


def case_id(c: dict) -> str:
    return "mixed" if c["kind"] == "mixed" else f"level{c['level']:g}-theta{c['theta_all']:g}-{c['spread']}"


# ---------------------------------------------------------------------------------------------------------------------
# dtheta's cancellation
# ---------------------------------------------------------------------------------------------------------------------

def sample_rate(c: dict) -> torch.Tensor:
    """V W exp(mean + scale eps) (E, D, N), the rate of the steps, in fp64."""
    return c["V"] * torch.matmul(c["W"], torch.exp(c["mean"] + c["scale"] * c["eps"]))


def theta_cancel(c: dict) -> torch.Tensor:
    """C_d = sum_n |psi(y + theta) - psi(theta)| + (1/E) sum_{e,n} (log1p(mu / theta) + |mu - y| / (mu + theta)): the sum
    of the absolute values of the summands of dtheta[d] (csrc/nb.hip's header), in fp64."""
    y, th, mu = c["y"], c["theta"][:, None], sample_rate(c)
    return (torch.digamma(y + th) - torch.digamma(th)).abs().sum(1) + \
        (torch.log1p(mu / th) + (mu - y).abs() / (mu + th)).sum((0, 2)) / mu.shape[0]


# ---------------------------------------------------------------------------------------------------------------------
# oracle, plain fp32 evaluation, bounds
# ---------------------------------------------------------------------------------------------------------------------

def _as_poisson(c: dict) -> dict:
    key = ("poisson-view", id(c))
    if key not in _cases:
        _cases[key] = dict(c, y=c["yp"])               # kept: the deviance oracles cache on the identity of c["y"]
    return _cases[key]


def _t(x) -> torch.Tensor:
    return torch.as_tensor(x, dtype=torch.float64)


def _step_f32(c: dict, y64: torch.Tensor, nb: bool) -> dict:
    """A step with fp32 element-wise arithmetic and fp64 sums, by the formulas of csrc/poisson.hip and csrc/nb.hip as they
    are written down (G = y / Z - V (y + theta) / (mu + theta), no rearrangement); lgamma(y + theta) - lgamma(theta) and the
    digamma terms in fp64."""
    f32, f64 = torch.float32, torch.float64
    mean, scale, eps, W, V, y = (t.to(f32) for t in (c["mean"], c["scale"], c["eps"], c["W"], c["V"], y64))
    expF = torch.exp(mean + scale * eps)                                                   # (E, Lt, N)
    Z = torch.einsum("dl,eln->edn", W.to(f64), expF.to(f64)).to(f32)
    mu = V * Z
    ne = expF.shape[0]
    if nb:
        th = c["theta"].to(f32)[:, None]
        t = (y + th) / (mu + th)
        l1p = torch.log1p(mu / th)
        th64 = c["theta"][:, None]
        val = (y * (torch.log(mu) - torch.log(th)) - (y + th) * l1p).to(f64).sum() / ne + \
            (torch.lgamma(y64 + th64) - torch.lgamma(th64)).sum()
        G, dv = y / Z - V * t, y / V - Z * t
        dth = (-l1p + (mu - y) / (mu + th)).to(f64).sum((0, 2)) / ne + (torch.digamma(y64 + th64) - torch.digamma(th64)).sum(1)
    else:
        val = (y * torch.log(mu) - mu).to(f64).sum() / ne
        G, dv = y / Z - V, y / V - Z
    G = G.to(f64) / ne
    dexp = torch.einsum("dl,edn->eln", W.to(f64), G) * expF.to(f64)
    out = dict(ll=val, ll_lgamma=val - torch.lgamma(y + 1.0).to(f64).sum(), dmean=dexp.sum(0),
               dscale=(dexp * eps.to(f64)).sum(0), dW=torch.einsum("edn,eln->dl", G, expF.to(f64)), dV=dv.to(f64).sum((0, 1)) / ne)
    if nb:
        out["dtheta"] = dth
    return out


def _blockwise(ref: torch.Tensor, blocks) -> torch.Tensor:
    """G_RTOL |ref| + G_ATOL max|ref|, the max over the genes (rows) of the same block; over everything without blocks."""
    a = ref.abs()
    if blocks is None:
        return G_RTOL * a + G_ATOL * a.max()
    m = torch.zeros(a.shape[0], dtype=torch.float64)
    for b in blocks.unique():
        m[blocks == b] = a[blocks == b].max()
    return G_RTOL * a + G_ATOL * m.reshape([-1] + [1] * (a.dim() - 1))


_evaluations: dict = {}


def evaluation(c: dict, family: str) -> dict:
    """dict(ref=, f32=, bound=): per output the fp64 oracle, the plain fp32 evaluation and the element-wise bound (fp64 CPU
    tensors, 0-d for the scalars).  Cached per case and shared by the tests: do not modify what it returns."""
    key = (id(c), family)
    if key in _evaluations:
        return _evaluations[key]
    assert family in FAMILIES
    poisson = family.startswith("poisson")
    blocks = c["poisson_blocks"] if poisson else c["blocks"]
    if family == "poisson_step":
        pc = _as_poisson(c)
        r = PC.reference(pc, False)
        lg = float(torch.lgamma(pc["y"] + 1.0).sum())
        ref = dict({k: r[k] for k in STEP_GRADS}, ll=_t(r["ll"]), ll_lgamma=_t(r["ll"] - lg))
        f32 = _step_f32(c, pc["y"], nb=False)
        bound = {k: PC.tolerance(r, k) for k in ("ll",) + STEP_GRADS}
    elif family == "nb_step":
        ll, g = NB.oracle({k: c[k].clone() for k in ("mean", "scale", "eps", "W", "V", "theta", "y")}, with_lgamma=False)
        lg = float(torch.lgamma(c["y"] + 1.0).sum())
        ref = dict({"d" + k: v for k, v in g.items()}, ll=_t(ll), ll_lgamma=_t(ll - lg))
        f32 = _step_f32(c, c["y"], nb=True)
        bound = {k: G_ATOL * (float(ref[k].abs().max()) + 1e-30) + G_RTOL * ref[k].abs() for k in STEP_GRADS}   # nb_cases.check
        bound["ll"] = _t(max(LL_REL * abs(ll), LL_ABS))
        bound["dtheta"] = G_RTOL * ref["dtheta"].abs() + G_ATOL * theta_cancel(c)
    else:
        mod, cc = (DC, _as_poisson(c)) if poisson else (NDC, c)
        ref, f32 = mod.oracle(cc, True), mod.fp32_evaluation(cc, True)
        bound = {k: mod.tolerance(ref, k) for k in OUTPUTS[family]}
    if "ll" in ref:
        bound["ll_lgamma"] = _t(LL_REL * (abs(float(ref["ll"])) + lg) + LL_ABS)
    if blocks is not None:
        for k in PER_GENE:
            if k in ref and k != "dtheta":
                bound[k] = _blockwise(ref[k], blocks)
    out = dict(ref=ref, f32={k: _t(f32[k]) for k in OUTPUTS[family]}, bound=bound)
    _evaluations[key] = out
    return out


def figure(got, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """The largest |got - ref| / bound; 0 where the error is 0 (so an output whose oracle and bound are both 0 must be
    exactly 0), inf for a value that is not finite."""
    g = torch.as_tensor(got).detach().double().cpu()
    assert g.shape == ref.shape, (g.shape, ref.shape)
    if not bool(torch.isfinite(g).all()):
        return float("inf")
    err = (g - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


def f32_figures(c: dict, family: str) -> dict:
    ev = evaluation(c, family)
    return {k: figure(ev["f32"][k], ev["ref"][k], ev["bound"][k]) for k in OUTPUTS[family]}


def in_domain(c: dict, family: str) -> dict:
    return {k: v <= IN_DOMAIN for k, v in f32_figures(c, family).items()}


def allowed(c: dict, family: str, name: str) -> torch.Tensor:
    """The element-wise bound of the GPU comparison: the bound for an output of the floor or in domain; max(bound,
    4 x |f32 - ref|) otherwise."""
    ev = evaluation(c, family)
    if name in floor(c, family) or in_domain(c, family)[name]:
        return ev["bound"][name]
    return torch.maximum(ev["bound"][name], OUT_OF_DOMAIN_MARGIN * (ev["f32"][name] - ev["ref"][name]).abs())


def floor(c: dict, family: str) -> tuple:
    """The outputs that must be in domain (a condition on the cases, not a measurement)."""
    if c["kind"] == "mixed" or family in ("poisson_step", "poisson_deviance"):
        return OUTPUTS[family]
    lv, th, wide = c["level"], c["theta_all"], c["spread"] == "wide"
    if family == "nb_step":
        return OUTPUTS[family] if lv / th <= 1e2 * (1 + 1e-9) else ("ll", "ll_lgamma", "dtheta")
    ok = (lv <= 1 and (th >= 1 or not wide)) or (lv == 1e2 and th >= 1 and not wide)
    return OUTPUTS[family] if ok else ()


# Where the plain fp32 evaluation itself misses a third of the bound although the floor names the output, at every seed:
# a count within sqrt(mu) of a rate of 1e4 has a unit deviance of about 1, while fp32 rounds y log y ~ 1e5 to 0.008, so
# y (log y - log mu) - y + mu by the two logarithms keeps two digits.  The Poisson entries' counts at level 1e4 are such
# counts throughout (gamma-Poisson counts at theta = 1e2 scatter by 10 % of mu and are not), and in the mixed case the genes
# at level 1e2 reach a rate of 1e4 under the spots with V near 1e2, which carry the per-spot sums.  The floor stands for the
# kernels all the same (``allowed`` gives them the plain bound); only the classification of the CPU evaluation is excused,
# for exactly these outputs.
F32_SHORT = {("poisson_deviance", "level10000-theta100-narrow"): ("per_gene", "per_spot", "total"),
             ("poisson_deviance", "mixed"): ("per_spot", "total"),
             ("nb_deviance", "mixed"): ("per_spot",)}


def missed_floor(c: dict, family: str) -> list:
    """The floor's outputs whose fp32 evaluation is out of domain, without those of F32_SHORT."""
    dom = in_domain(c, family)
    return [k for k in floor(c, family) if not dom[k] and k not in F32_SHORT.get((family, case_id(c)), ())]


NB_IDS = [f"level{lv:g}-theta{th:g}-{sp}" for lv, th, sp in NB_GRID] + ["mixed"]
POISSON_IDS = [f"level{lv:g}-theta{th:g}-{sp}" for lv, th, sp in POISSON_GRID] + ["mixed"]


def lookup(cid: str) -> dict:
    """The case of an id of NB_IDS / POISSON_IDS, built on first use."""
    if cid == "mixed":
        return mixed_case()
    return regime_case(*NB_GRID[NB_IDS.index(cid)])
