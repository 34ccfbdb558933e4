"""Cases, the fp64 oracle and the fp32 emulation for tests/test_hip_residual_autocorr.py (TEST INFRASTRUCTURE ONLY; numpy and
plain torch, importable without a GPU -- tests/test_residual_cases.py checks everything here on the CPU).

The operation is csrc/residual.hip: residuals of counts under the predictive mean rate of a fitted count model and Moran's I
of every gene's residuals over a neighbour table,

    m = exp(mean + scale^2 / 2),   mu = V W m,
    Pearson   r = (y - mu) / sqrt(mu (1 + mu / theta))                      (Poisson: theta = inf)
    deviance  r = sign(y - mu) sqrt(max(d, 0)),  d = 2 (y log(y / mu) - (y - mu))                               (Poisson)
                                                 d = 2 [y log(y / mu) - (y + theta) log1p((y - mu) / (mu + theta))]   (NB)
    I = sum_n z_n (1 / K) sum_k z_nbr[n,k] / sum_n z_n^2,  z = r - mean(r).

The reference has no such function; the oracle is these formulas in fp64 numpy on the same fp32-representable inputs.

TOLERANCES.  A residual passes with |got - ref| <= RTOL |ref| + ATOL.  Neither number was fixed in advance: ``measure()``
runs the CPU emulation of the kernel's fp32 element-wise arithmetic (``emulate_residuals``: the kernel's own forms, every
operation rounded to fp32 by torch) against the oracle over every case x kind x family of the table below, and
    RTOL = 3 x the worst |err| / |ref| over the elements with |ref| >= 1,
    ATOL = 3 x the worst |err|         over the elements with |ref| <  1,
each rounded up to one significant digit; so an element with |ref| >= 1 is held to RTOL |ref| alone and a smaller one to
ATOL alone, whatever the other term adds.  Measured (this table, seed 0 of every case):
    worst relative error, |ref| >= 1:  9.52e-06  (Poisson deviance residual, case lt56)
    worst absolute error, |ref| <  1:  1.36e-05  (NB deviance residual, case lt64_block_edge)
so RTOL = 3e-5 and ATOL = 5e-5.  RTOL EXCEEDS deviance_cases.G_RTOL (2e-5), and ATOL, an absolute bound on one residual of
order 1, has no counterpart there (G_ATOL scales with max|ref| of a sum).  The term behind both is y - mu where a count
lies next to a large rate: mu is an fp32 dot product of up to 64 factors times V, off by a few 2^-24 mu (1e-5 at the
mu ~ 50..2000 of the spots with V = BIG_SIZE), while |y - mu| is of order sqrt(mu), so the residual inherits
err(mu) / sqrt(mu) absolutely and err(mu) / |y - mu| relatively, in either kind; the deviance kind adds the square root
next to y = mu, which halves the digits of d.  A deviance sums its terms and averages this error away; a residual is one
element and cannot.
``I`` end to end passes with |got - ref| <= I_ATOL: the emulated fp32 residuals pushed through the fp64 Moran oracle against
the oracle's own over ``case_table`` of every case, worst 2.85e-07 (case lt56), x 3 and rounded up: I_ATOL = 9e-7.
``make_case`` redraws a case with the next seed if its emulation does not stay within a third of these; nothing is loosened.
"""
from __future__ import annotations

import math

import numpy as np
import torch

RTOL = 3e-5
ATOL = 5e-5
I_ATOL = 9e-7

KINDS = ("pearson", "deviance")
FAMILIES = ("poisson", "nb")
THETA_RANGE = (0.05, 1e7)
BIG_COUNT = 5000.0            # y >> mu
BIG_SIZE = 30.0               # V at the spots of the zero probes: y = 0 beside mu >> 1

# (name, D, B, Lt, why)
TABLE = (
    ("one_gene", 1, 7, 1, "one gene, one partial tile, one factor: every mask at once"),
    ("odd_small", 17, 63, 3, "a partial wave of genes and a tile short by one spot; Lt not a multiple of 4"),
    ("exact_block", 64, 64, 4, "exactly one gene block and one tile: no masked lane anywhere; vector loads of y"),
    ("one_past", 65, 65, 5, "one gene and one spot past a block and a tile; rows of y not 16-byte aligned"),
    ("two_blocks", 130, 130, 8, "three gene blocks, three tiles, the last of each partial; 2 k-steps"),
    ("long_rows", 33, 257, 9, "five tiles, the last holding one spot; 3 k-steps"),
    ("lt20", 130, 257, 20, "the flagship factor count (5 k-steps) over several blocks and tiles"),
    ("lt33", 64, 130, 33, "9 k-steps: the first instance that loads the A operand inside the loop"),
    ("lt64_block_edge", 65, 64, 64, "the largest factor count (16 k-steps), one gene past a block"),
    # the k-step instances the shapes above do not reach (4, 6, 7, 8, 10, 12, 14 k-steps)
    ("lt16", 17, 70, 16, "4 k-steps"),
    ("lt24", 17, 70, 24, "6 k-steps"),
    ("lt28", 17, 70, 28, "7 k-steps"),
    ("lt32", 17, 70, 32, "8 k-steps: the last instance that prefetches the A operand"),
    ("lt40", 17, 70, 40, "10 k-steps"),
    ("lt45", 17, 70, 45, "12 k-steps, padded from 45 factors"),
    ("lt56", 17, 70, 56, "14 k-steps"),
)
K_STEPS = {1: 1, 3: 1, 4: 1, 5: 2, 8: 2, 9: 3, 20: 5, 33: 9, 64: 16, 16: 4, 24: 6, 28: 7, 32: 8, 40: 10, 45: 12, 56: 14}
ALL_K_STEPS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16)


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# oracle (fp64 numpy)
# ---------------------------------------------------------------------------------------------------------------------

def rate(c, lognormal_mean=True):
    m = np.exp(c["mean"] + (0.5 * c["scale"] ** 2 if lognormal_mean else 0.0))
    return c["V"][None, :] * (c["W"] @ m)


def _ylog(y, mu):
    pos = y > 0
    return np.where(pos, y * np.log(np.where(pos, y, 1.0) / mu), 0.0)


def unit_deviance(y, mu, theta=None):
    """The issue's formulas, not clamped."""
    if theta is None:
        return 2.0 * (_ylog(y, mu) - (y - mu))
    th = theta[:, None]
    return 2.0 * (_ylog(y, mu) - (y + th) * np.log1p((y - mu) / (mu + th)))


def unit_deviance_nb_split(y, mu, theta):
    """The NB deviance as 2 (y A - theta B): A = log(y (mu + theta) / (mu (y + theta))), B = log((y + theta) / (mu + theta))."""
    th = theta[:, None]
    pos = y > 0
    A = np.where(pos, np.log(np.where(pos, y, 1.0) * (mu + th) / (mu * (y + th))), 0.0)
    return 2.0 * (y * A - th * np.log((y + th) / (mu + th)))


def residuals(y, mu, kind, theta=None):
    """(D, B) fp64 residuals; theta None: Poisson."""
    if kind == "pearson":
        var = mu if theta is None else mu * (1.0 + mu / theta[:, None])
        return (y - mu) / np.sqrt(var)
    assert kind == "deviance"
    return np.sign(y - mu) * np.sqrt(np.maximum(unit_deviance(y, mu, theta), 0.0))


def theta_of(c, family):
    assert family in FAMILIES
    return c["theta"] if family == "nb" else None


_oracle_cache: dict = {}


def oracle_residuals(c, kind, family):
    """Cached and shared by the tests: do not modify what it returns."""
    key = (c["name"], c["seed"], kind, family)
    if key not in _oracle_cache:
        _oracle_cache[key] = residuals(c["y"], rate(c), kind, theta_of(c, family))
    return _oracle_cache[key]


def morans_i(R, nbr):
    """Moran's I, the residual mean and variance of every row of R (G, B) over nbr (B, K), written out as the double sum."""
    R = np.asarray(R, dtype=np.float64)
    mean = R.mean(axis=1)
    z = R - mean[:, None]
    K = nbr.shape[1]
    num = np.zeros(R.shape[0])
    for k in range(K):
        num += (z * z[:, nbr[:, k]]).sum(axis=1) / K
    den = (z * z).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return num / den, mean, den / R.shape[1]


# ---------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernel's element-wise arithmetic (torch rounds every operation to fp32)
# ---------------------------------------------------------------------------------------------------------------------

_LN2 = 0.69314718055994530942


def _log1p_c(x):
    u = 1.0 + x
    big = _LN2 * torch.log2(u) + (x - (u - 1.0)) / u
    small = x * (x * (x * (1.0 / 3.0) - 0.5) + 1.0)
    return torch.where(x < 2.0 ** -12, small, big)


def _pois_dev32(y, mu):
    pos, up = y > 0, y >= mu
    ys = torch.where(pos, y, torch.ones_like(y))
    l = _log1p_c((ys - mu).abs() / torch.where(up, mu, ys))
    t = torch.where(pos, torch.where(up, y * l, -y * l), torch.zeros_like(y))
    return 2.0 * (t - (y - mu))


def _nb_dev32(y, mu, th):
    up, pos = y >= mu, y > 0
    d = (y - mu).abs()
    lo, hi = torch.where(up, mu, y), torch.where(up, y, mu)
    b = _log1p_c(d / (lo + th))
    a = _log1p_c(th * d / (torch.where(pos, lo, torch.ones_like(lo)) * (hi + th)))
    ya, tb = torch.where(pos, y * a, torch.zeros_like(y)), th * b
    return 2.0 * torch.where(up, ya - tb, tb - ya)


def emulate_residuals(c, kind, family):
    """(D, B) fp64 array of the residuals with fp32 element-wise arithmetic in the kernel's forms."""
    f32 = torch.float32
    t = {k: torch.tensor(c[k], dtype=f32) for k in ("mean", "scale", "W", "V", "y", "theta")}
    m = torch.exp(t["mean"] + 0.5 * t["scale"] * t["scale"])
    z = torch.zeros_like(t["y"])
    for l in range(c["Lt"]):                        # the factors in order, one rounding per product and per sum: no BLAS,
        z = z + t["W"][:, l:l + 1] * m[l:l + 1, :]  # whose order of summation would depend on the host
    mu = t["V"] * z
    y, th = t["y"], t["theta"][:, None]
    e = y - mu
    if kind == "pearson":
        var = mu * (mu * (1.0 / th) + 1.0) if family == "nb" else mu
        r = e * torch.rsqrt(var)
    else:
        d = _nb_dev32(y, mu, th) if family == "nb" else _pois_dev32(y, mu)
        s = torch.sqrt(d.clamp(min=0.0))
        r = torch.where(e < 0, -s, s)
    return r.double().numpy()


def residual_errors(ref, got):
    """(worst |err| / |ref| over |ref| >= 1, worst |err| over |ref| < 1)."""
    err, big = np.abs(got - ref), np.abs(ref) >= 1.0
    rel = float((err[big] / np.abs(ref[big])).max()) if big.any() else 0.0
    ab = float(err[~big].max()) if (~big).any() else 0.0
    return rel, ab


def residual_figure(ref, got):
    """The largest |got - ref| / (RTOL |ref| + ATOL); inf if a value is not finite."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / (RTOL * np.abs(ref) + ATOL)).max())


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------

def probe_positions(D, B):
    """(gene, spot) pairs at the first and last spot of a tile of 64 and at the last gene of a wave (16), a block (64) and the
    array (the last gene of a slab, whatever slab_genes divides it)."""
    genes = sorted({g for g in (0, 15, 16, 63, 64, 127, 128, D - 1) if 0 <= g < D})
    spots = sorted({s for s in (0, 63, 64, 127, 128, B - 1) if 0 <= s < B})
    return [(g, s) for g in genes for s in spots]


def random_table(B, K, seed=0):
    """(B, K) int64: K distinct neighbours per spot, drawn from the whole range (other tiles, other spot slices), no self."""
    rng = np.random.default_rng(1234 + seed)
    nbr = np.empty((B, K), dtype=np.int64)
    for n in range(B):
        pick = rng.choice(B - 1, size=K, replace=False)
        nbr[n] = np.where(pick >= n, pick + 1, pick)
    return nbr


def knn_table(X, K):
    """(N, K) int64 self-excluded nearest neighbours by (fp64 squared distance, index), the rule of ops.spatial_knn."""
    X = np.asarray(X, dtype=np.float64)
    d2 = np.zeros((X.shape[0], X.shape[0]))
    for k in range(X.shape[1]):
        diff = X[:, None, k] - X[None, :, k]
        d2 = d2 + diff * diff
    np.fill_diagonal(d2, np.inf)
    return np.argsort(d2, axis=1, kind="stable")[:, :K].astype(np.int64)


def _draw(name, D, B, Lt, seed):
    rng = np.random.default_rng([9000 + seed, D, B, Lt])
    c = dict(name=name, D=D, B=B, Lt=Lt, seed=seed,
             mean=0.5 * rng.standard_normal((Lt, B)), scale=0.2 + 0.5 * rng.random((Lt, B)),
             W=0.01 + 0.3 * np.exp(rng.standard_normal((D, Lt))), V=np.exp(0.7 * rng.standard_normal(B)))
    lo, hi = THETA_RANGE
    c["theta"] = rng.permutation(np.exp(np.linspace(math.log(lo), math.log(hi), D)))      # every decade, in no gene order
    probes = probe_positions(D, B)
    zero_spots = sorted({s for i, (g, s) in enumerate(probes) if i % 2})
    for s in zero_spots:
        c["V"][s] = BIG_SIZE
    for k in ("mean", "scale", "W", "V", "theta"):
        c[k] = _f32(c[k])
    c["y"] = rng.poisson(rate(c)).astype(np.float64)
    c["probes"] = []
    for i, (g, s) in enumerate(probes):
        c["y"][g, s] = 0.0 if i % 2 else BIG_COUNT + 37.0 * i
        c["probes"].append((g, s, c["y"][g, s]))
    return c


def within_a_third(c):
    for kind in KINDS:
        for family in FAMILIES:
            if residual_figure(oracle_residuals(c, kind, family), emulate_residuals(c, kind, family)) > 1.0 / 3.0:
                return False
    return True


_case_cache: dict = {}


def make_case(name):
    """The named case of TABLE (fp64 numpy arrays holding fp32-representable values), redrawn with the next seed until the
    emulation stays within a third of the residual tolerance.  Cached: do not modify what it returns."""
    if name not in _case_cache:
        row = next(r for r in TABLE if r[0] == name)
        for attempt in range(8):
            c = _draw(name, row[1], row[2], row[3], attempt)
            if within_a_third(c):
                _case_cache[name] = c
                break
        else:
            raise AssertionError(f"no draw of {name} keeps the fp32 emulation within a third of the tolerance")
    return _case_cache[name]


def i_error(c, nbr):
    """Worst |I(emulated residuals) - I(oracle residuals)| over kinds and families."""
    worst = 0.0
    for kind in KINDS:
        for family in FAMILIES:
            ref = morans_i(oracle_residuals(c, kind, family), nbr)[0]
            got = morans_i(emulate_residuals(c, kind, family), nbr)[0]
            worst = max(worst, float(np.abs(got - ref).max()))
    return worst


def case_table(c, K=None):
    """The random neighbour table a case is scored over end to end: K = 6, or B - 1 where there are fewer spots."""
    K = min(6, c["B"] - 1) if K is None else K
    return random_table(c["B"], K, seed=c["B"])


def measure():
    """Prints the figures RTOL, ATOL and I_ATOL are taken from (python tests/residual_cases.py)."""
    worst = [(0.0, ""), (0.0, ""), (0.0, "")]
    for name, *_ in TABLE:
        c = _draw(name, *next(r for r in TABLE if r[0] == name)[1:4], 0)
        for kind in KINDS:
            for family in FAMILIES:
                ref = residuals(c["y"], rate(c), kind, theta_of(c, family))
                rel, ab = residual_errors(ref, emulate_residuals(c, kind, family))
                worst[0] = max(worst[0], (rel, f"{name} {kind} {family}"))
                worst[1] = max(worst[1], (ab, f"{name} {kind} {family}"))
        worst[2] = max(worst[2], (i_error(c, case_table(c)), name))
    for label, (v, where) in zip(("relative, |ref| >= 1", "absolute, |ref| < 1", "I"), worst):
        print(f"worst {label}: {v:.3e} ({where}); x 3 = {3 * v:.3e}")


# ---------------------------------------------------------------------------------------------------------------------
# planted structure
# ---------------------------------------------------------------------------------------------------------------------

PLANTED_SEED = 0
PLANTED_GENES = (5, 14, 23, 32)


def planted_case(seed=PLANTED_SEED):
    """B = 400 spots on a 20 x 20 grid (jittered, so no distance ties), D = 40, Lt = 3.  Thirty-six genes are Poisson(mu);
    the genes PLANTED_GENES are Poisson(mu (1 + 0.8 s)), s = sin(2 pi x / 10): a smooth +-1 pattern of period half the grid
    that the model's rate does not contain."""
    rng = np.random.default_rng(77 + seed)
    gx, gy = np.meshgrid(np.arange(20.0), np.arange(20.0), indexing="ij")
    X = np.stack([gx.ravel(), gy.ravel()], axis=1) + 0.05 * rng.random((400, 2))
    D, B, Lt = 40, 400, 3
    c = dict(name="planted", seed=seed, D=D, B=B, Lt=Lt, X=_f32(X),
             mean=_f32(0.3 * rng.standard_normal((Lt, B))), scale=_f32(0.1 + 0.1 * rng.random((Lt, B))),
             W=_f32(1.0 + rng.random((D, Lt))), V=_f32(np.ones(B)), theta=_f32(np.full(D, 10.0)))
    mu = rate(c)
    s = np.sin(2.0 * np.pi * X[:, 0] / 10.0)
    planted = np.zeros(D, dtype=bool)
    planted[list(PLANTED_GENES)] = True
    c["y"] = rng.poisson(np.where(planted[:, None], mu * (1.0 + 0.8 * s[None, :]), mu)).astype(np.float64)
    c["planted"] = planted
    c["nbr"] = knn_table(c["X"], 6)
    return c


def moran_z(I, nbr):
    """z of gpzoo's residual_autocorr from I and the table: (I - expected) / sqrt(variance), the moments of
    gpzoo_amd.utilities._moran_moments."""
    from gpzoo_amd.utilities import _moran_moments
    expected, variance = _moran_moments(torch.as_tensor(nbr))
    return (np.asarray(I) - float(expected)) / math.sqrt(float(variance))


def planted_conditions(z, planted):
    """The three conditions of the planted case on a z vector."""
    z = np.asarray(z)
    top = set(np.argsort(-z)[:int(planted.sum())].tolist())
    return bool((z[planted] > 6).all()), bool((np.abs(z[~planted]) < 4).all()), top == set(np.flatnonzero(planted).tolist())


if __name__ == "__main__":
    measure()
