"""Cases, the fp64 oracle and the fp32 emulation for tests/test_hip_gaussian_residual.py (TEST INFRASTRUCTURE ONLY; numpy and
plain torch, importable without a GPU -- tests/test_gaussian_residual_cases.py checks everything here on the CPU).

The operation is csrc/residual_gaussian.h behind the driver of csrc/residual.hip: residuals of real-valued expression under a
fitted Gaussian factor model, q(F) = N(mean, scale^2), and the spatial autocorrelation of every gene's residuals,

    yhat = b[:, None] + W mean,           v = sd[:, None]^2 + W^2 scale^2,
    pearson     r = (y - yhat) / sd       response    r = y - yhat       predictive  r = (y - yhat) / sqrt(v)
    I = sum_n z_n (1 / K) sum_k z_nbr[n,k] / sum_n z_n^2,   C = (B - 1) sum_n sum_k (z_n - z_nbr[n,k])^2 / (2 B K sum_n z_n^2),
    z = r - mean(r).

The reference has no such function; the oracle is these formulas in fp64 numpy on the same fp32-representable inputs.

EMULATION.  ``emulate_residuals`` is the kernel's own element-wise order with every operation rounded to fp32: the product
W mean as the k-ordered fused multiply-add chain v_mfma_f32_16x16x4_f32 computes (factors ascending, one rounding per step;
the fp32 fma is formed as an exact fp64 product plus an fp64 sum rounded to fp32, which differs from a true fma only in rare
double roundings), W^2 and scale^2 squared in fp32 first, then e = y - (b + z), e / sd, e / sqrt(sd sd + z2) with the
correctly rounded division and square root.

TOLERANCE.  The error of y - yhat scales with the size of its terms, not with the residual, so an element passes with
    |got - ref| <= RTOL |ref| + CTOL 2^-24 S / den,     S = |y| + |b| + sum_l |W[d,l] mean[l,n]|,
den the kind's denominator (sd, 1, sqrt(v)).  Neither number was fixed in advance; ``measure()`` takes each from the
emulation over every case x kind of the table (seed 0 of every case), one term at a time:
    CTOL = 3 x the worst |e_emulated - e_oracle| / (2^-24 S) of the numerator e = y - yhat (it is the response residual:
           that kind has no other error), and
    RTOL = 3 x the worst relative error the standardisation adds to the emulated numerator,
           |r_emulated - e_emulated / den_oracle| / |e_emulated / den_oracle|, over the pearson and predictive kinds,
each rounded up to one significant digit.  Measured:
    worst numerator figure:        3.118 (case lt33)                               so CTOL = 1e1
    worst standardisation figure:  2.702e-07 (predictive, case lt64_block_edge)    so RTOL = 9e-7
I and C end to end pass with |got - ref| <= I_ATOL / C_ATOL: the emulated fp32 residuals pushed through the fp64 oracle of I
and C against the oracle's own over ``case_table`` of every case and kind, worst
    I: 4.645e-06 (case lt64_block_edge)     C: 5.741e-06 (case lt45),
x 3 and rounded up: I_ATOL = 2e-5, C_ATOL = 2e-5.  These are far above residual_cases.I_ATOL (9e-7): a gene with sd = 1e-2
has residuals of 1e-2 in data units beside terms of y - yhat of size 5, so fp32 leaves it four digits, whatever the kind.
``make_case`` redraws a case with the next seed if its emulation does not stay within a third of these, at most three
draws; no case and no element is ever left out, nothing is loosened.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from residual_cases import ALL_K_STEPS, K_STEPS, TABLE, knn_table, probe_positions, random_table  # noqa: F401

RTOL = 9e-7
CTOL = 1e1
I_ATOL = 2e-5
C_ATOL = 2e-5

KINDS = ("pearson", "response", "predictive")
U = 2.0 ** -24
MAX_DRAWS = 3
SD_RANGE = (1e-2, 1e2)
PROBE = 300.0                 # |y| at the probes, beside yhat of order 1


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# oracle (fp64 numpy)
# ---------------------------------------------------------------------------------------------------------------------

def predictive_mean(c):
    return c["b"][:, None] + c["W"] @ c["mean"]


def predictive_var(c):
    return c["sd"][:, None] ** 2 + (c["W"] ** 2) @ (c["scale"] ** 2)


def denominator(c, kind):
    if kind == "pearson":
        return np.broadcast_to(c["sd"][:, None], (c["D"], c["B"]))
    if kind == "response":
        return np.ones((c["D"], c["B"]))
    assert kind == "predictive"
    return np.sqrt(predictive_var(c))


def residuals(c, kind, y=None):
    """(D, B) fp64 residuals: the formulas of the module docstring."""
    y = c["y"] if y is None else y
    return (y - predictive_mean(c)) / denominator(c, kind)


def term_size(c, y=None):
    """S = |y| + |b| + sum_l |W mean|, the size of the terms of y - yhat."""
    y = c["y"] if y is None else y
    return np.abs(y) + np.abs(c["b"])[:, None] + np.abs(c["W"]) @ np.abs(c["mean"])


_oracle_cache: dict = {}


def oracle_residuals(c, kind):
    """Cached and shared by the tests: do not modify what it returns."""
    key = (c["name"], c["seed"], kind)
    if key not in _oracle_cache:
        _oracle_cache[key] = residuals(c, kind)
    return _oracle_cache[key]


def spatial_stats(R, nbr):
    """I, C, mean, variance (sum z^2 / B) and kurtosis (m4 / m2^2) of every row of R (G, B) over nbr (B, K), as double sums."""
    R = np.asarray(R, dtype=np.float64)
    B, K = nbr.shape
    mean = R.mean(axis=1)
    z = R - mean[:, None]
    num, gnum = np.zeros(R.shape[0]), np.zeros(R.shape[0])
    for k in range(K):
        zk = z[:, nbr[:, k]]
        num += (z * zk).sum(axis=1) / K
        gnum += ((z - zk) ** 2).sum(axis=1)
    den = (z * z).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return dict(I=num / den, C=(B - 1) * gnum / (2.0 * B * K * den), residual_mean=mean, residual_var=den / B,
                    kurtosis=((z ** 4).sum(axis=1) / B) / (den / B) ** 2)


# ---------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernel's arithmetic
# ---------------------------------------------------------------------------------------------------------------------

def _fma_chain(W, A):
    """sum_l W[:, l] A[l, :] as the k-ordered fp32 fma chain of the MFMA: (D, B) float32."""
    z = np.zeros((W.shape[0], A.shape[1]), dtype=np.float32)
    W64, A64 = W.astype(np.float64), A.astype(np.float64)
    for l in range(W.shape[1]):
        z = (A64[l][None, :] * W64[:, l][:, None] + z.astype(np.float64)).astype(np.float32)
    return z


def emulate_parts(c, y=None):
    """(e, sd, sqrt(v)) in float32 as the kernel forms them: the numerator y - (b + z) and the two denominators."""
    f = np.float32
    W, m, s = c["W"].astype(f), c["mean"].astype(f), c["scale"].astype(f)
    b, sd = c["b"].astype(f)[:, None], c["sd"].astype(f)[:, None]
    y = (c["y"] if y is None else y).astype(f)
    e = y - (b + _fma_chain(W, m))
    z2 = _fma_chain(W * W, s * s)
    return e, sd, np.sqrt(sd * sd + z2)


def emulate_residuals(c, kind, y=None):
    """(D, B) fp64 array of the residuals with the kernel's fp32 arithmetic."""
    e, sd, rv = emulate_parts(c, y)
    r = e if kind == "response" else e / sd if kind == "pearson" else e / rv
    assert r.dtype == np.float32
    return r.astype(np.float64)


def tolerance(c, kind, y=None):
    """The element-wise bound RTOL |ref| + CTOL 2^-24 S / den, (D, B)."""
    return RTOL * np.abs(residuals(c, kind, y)) + CTOL * U * term_size(c, y) / denominator(c, kind)


def residual_figure(c, kind, got, y=None):
    """The largest |got - ref| / tolerance; inf if a value is not finite."""
    got = np.asarray(got, dtype=np.float64)
    ref = oracle_residuals(c, kind) if y is None else residuals(c, kind, y)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / tolerance(c, kind, y)).max())


def term_figures(c):
    """(worst numerator figure |e_emu - e_ref| / (2^-24 S), worst standardisation figure with its kind) of one draw."""
    e, sd, rv = emulate_parts(c)
    e64 = e.astype(np.float64)
    num = float((np.abs(e64 - residuals(c, "response")) / (U * term_size(c))).max())
    worst = (0.0, "")
    for kind, r in (("pearson", e / sd), ("predictive", e / rv)):
        want = e64 / denominator(c, kind)
        ok = want != 0
        worst = max(worst, (float((np.abs(r.astype(np.float64) - want)[ok] / np.abs(want[ok])).max()), kind))
    return num, worst


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------

def _draw(name, D, B, Lt, seed):
    rng = np.random.default_rng([7100 + seed, D, B, Lt])
    scale = 1.2 * rng.random((Lt, B)) ** 2
    scale[:, rng.random(B) < 0.25] = 0.0            # spots where q(F) is a point: predictive = pearson there
    sd = np.exp(np.linspace(math.log(SD_RANGE[0]), math.log(SD_RANGE[1]), D)) if D > 1 else np.array([SD_RANGE[0]])
    c = dict(name=name, D=D, B=B, Lt=Lt, seed=seed, mean=0.7 * rng.standard_normal((Lt, B)), scale=scale,
             W=0.5 * rng.standard_normal((D, Lt)), b=2.0 * rng.standard_normal(D), sd=rng.permutation(sd))
    for k in ("mean", "scale", "W", "b", "sd"):
        c[k] = _f32(c[k])
    y = predictive_mean(c) + c["sd"][:, None] * rng.standard_normal((D, B))
    c["probes"] = []
    for i, (g, s) in enumerate(probe_positions(D, B)):
        y[g, s] = (-1.0 if i % 2 else 1.0) * (PROBE + 37.0 * i)
        c["probes"].append((g, s, y[g, s]))
    c["y"] = _f32(y)
    return c


def case_table(c, K=None):
    """The random neighbour table a case is scored over end to end: K = 6, or B - 1 where there are fewer spots."""
    K = min(6, c["B"] - 1) if K is None else K
    return random_table(c["B"], K, seed=c["B"])


def stat_errors(c):
    """Worst |I(emulated) - I(oracle)| and |C(emulated) - C(oracle)| over the kinds."""
    nbr, wi, wc = case_table(c), 0.0, 0.0
    for kind in KINDS:
        ref, got = spatial_stats(residuals(c, kind), nbr), spatial_stats(emulate_residuals(c, kind), nbr)
        wi, wc = max(wi, float(np.abs(got["I"] - ref["I"]).max())), max(wc, float(np.abs(got["C"] - ref["C"]).max()))
    return wi, wc


def within_a_third(c):
    if any(residual_figure(c, kind, emulate_residuals(c, kind), y=c["y"]) > 1.0 / 3.0 for kind in KINDS):
        return False
    wi, wc = stat_errors(c)
    return wi <= I_ATOL / 3.0 and wc <= C_ATOL / 3.0


_case_cache: dict = {}
draws_used: dict = {}


def make_case(name):
    """The named case of TABLE (fp64 numpy arrays holding fp32-representable values), redrawn with the next seed until the
    emulation stays within a third of the tolerances, at most MAX_DRAWS draws.  Cached: do not modify what it returns."""
    if name not in _case_cache:
        row = next(r for r in TABLE if r[0] == name)
        for attempt in range(MAX_DRAWS):
            c = _draw(name, row[1], row[2], row[3], attempt)
            if within_a_third(c):
                _case_cache[name], draws_used[name] = c, attempt + 1
                break
        else:
            raise AssertionError(f"no draw of {name} keeps the fp32 emulation within a third of the tolerance")
    return _case_cache[name]


def measure():
    """Prints the figures RTOL, CTOL, I_ATOL and C_ATOL are taken from (python tests/gaussian_residual_cases.py)."""
    worst = [(0.0, ""), (0.0, ""), (0.0, ""), (0.0, "")]
    for name, D, B, Lt, _ in TABLE:
        c = _draw(name, D, B, Lt, 0)
        num, (rel, kind) = term_figures(c)
        wi, wc = stat_errors(c)
        worst = [max(worst[0], (num, name)), max(worst[1], (rel, f"{kind}, {name}")), max(worst[2], (wi, name)),
                 max(worst[3], (wc, name))]
    for label, (v, where) in zip(("numerator figure (CTOL)", "standardisation figure (RTOL)", "I", "C"), worst):
        print(f"worst {label}: {v:.3e} ({where}); x 3 = {3 * v:.3e}")


# ---------------------------------------------------------------------------------------------------------------------
# expression stored as its non-zeros
# ---------------------------------------------------------------------------------------------------------------------

SPARSE_CASES = ("rows", "holes")
OFFSETS = ("centred", "uncentred")


def sparse_case(which, offset):
    """A case whose data are values - offset with the values mostly zero: (case with y = the dense fp32 array, values (D, B)
    fp64 holding fp32 values, offset (D,) fp64).  "rows" (6 x 600, Lt = 5): rows of 511, 512 and 513 stored entries and an
    entry at the last spot of the first gene.  "holes" (130 x 130, Lt = 8): a gene without stored entries and a gene stored at
    every spot.  ``offset``: "centred" (the row means of the values, what log_normalize gives) or "uncentred" (arbitrary
    offsets of both signs, 0 for one gene and 50 for another)."""
    rng = np.random.default_rng(5)
    if which == "rows":
        c = dict(_draw("rows", 6, 600, 5, 0))
        v = np.log1p(rng.poisson(3.0, (6, 600))) * (rng.random((6, 600)) < 0.05)
        for g, n in ((1, 511), (2, 512), (3, 513)):
            v[g] = 0.0
            v[g, rng.permutation(600)[:n]] = np.log1p(1.0 + rng.poisson(3.0, n))
        v[0, 599] = 7.0
    else:
        assert which == "holes"
        c = dict(make_case("two_blocks"))
        c["name"] = "holes"
        v = np.log1p(rng.poisson(3.0, (130, 130))) * (rng.random((130, 130)) < 0.3)
        v[17] = 0.0
        v[64] = 0.5 + rng.random(130)
        v[129, 129] = 300.0
    v = _f32(v)
    if offset == "centred":
        off = v.mean(axis=1)
    else:
        assert offset == "uncentred"
        off = 3.0 * rng.standard_normal(v.shape[0])
        off[0], off[1] = 0.0, 50.0
    c["y"] = (v - off[:, None]).astype(np.float32).astype(np.float64)     # what SparseExpression.to_dense() holds
    c["probes"] = []
    return c, v, off


def sparse_expression(v, off, device="cpu"):
    from gpzoo.likelihoods import SparseCounts, SparseExpression
    return SparseExpression(SparseCounts(torch.tensor(v, dtype=torch.float32, device=device)),
                            torch.tensor(off, dtype=torch.float64, device=device))


# ---------------------------------------------------------------------------------------------------------------------
# planted structure
# ---------------------------------------------------------------------------------------------------------------------

PLANTED_SEED = 1                              # the first seed at which no other gene ties the smallest attainable p-value,
PLANTED_GENES = tuple(range(4, 100, 10))      # 1 / 200, under the fp64 oracle (seed 0 has such a gene); 10 of 100
PLANTED_PERMS = 199


def planted_case(seed=PLANTED_SEED):
    """B = 400 spots on a jittered 20 x 20 grid, D = 100, Lt = 3.  Every gene is yhat + sd noise under a rank-3 model; the
    genes PLANTED_GENES carry one extra smooth factor, a sin(2 pi x / 10) of amplitude 1.5 sd, which the model does not
    contain.  ``perms``: the PLANTED_PERMS relabellings the test scores (drawn here, so the p-values are the same wherever
    they are computed)."""
    rng = np.random.default_rng(177 + seed)
    gx, gy = np.meshgrid(np.arange(20.0), np.arange(20.0), indexing="ij")
    X = np.stack([gx.ravel(), gy.ravel()], axis=1) + 0.05 * rng.random((400, 2))
    D, B, Lt = 100, 400, 3
    c = dict(name="planted", seed=seed, D=D, B=B, Lt=Lt, X=_f32(X), mean=_f32(0.7 * rng.standard_normal((Lt, B))),
             scale=_f32(0.1 + 0.1 * rng.random((Lt, B))), W=_f32(0.5 * rng.standard_normal((D, Lt))),
             b=_f32(rng.standard_normal(D)), sd=_f32(np.exp(rng.uniform(-1.0, 1.0, D))))
    planted = np.zeros(D, dtype=bool)
    planted[list(PLANTED_GENES)] = True
    extra = np.sin(2.0 * np.pi * X[:, 0] / 10.0)
    y = predictive_mean(c) + c["sd"][:, None] * (rng.standard_normal((D, B)) + 1.5 * planted[:, None] * extra[None, :])
    c["y"], c["planted"], c["nbr"] = _f32(y), planted, knn_table(c["X"], 6)
    c["perms"] = np.stack([rng.permutation(B) for _ in range(PLANTED_PERMS)]).astype(np.int64)
    return c


def permutation_pvalues(R, nbr, perms):
    """(pval_greater of I, pval_less of C) of every row of R under the relabellings r^pi[n] = r[pi[n]], fp64 numpy."""
    obs = spatial_stats(R, nbr)
    n_ge, n_le = np.zeros(R.shape[0]), np.zeros(R.shape[0])
    for p in perms:
        sim = spatial_stats(R[:, p], nbr)
        n_ge += sim["I"] >= obs["I"]
        n_le += sim["C"] <= obs["C"]
    return (n_ge + 1.0) / (len(perms) + 1.0), (n_le + 1.0) / (len(perms) + 1.0)


def planted_found(pval, planted):
    """The planted genes have the smallest p-values: every one of them below every other gene's."""
    pval = np.asarray(pval)
    return bool(pval[planted].max() < pval[~planted].min())


if __name__ == "__main__":
    measure()
